"""Scene branch on MI355X: drop-in for the reference's `NeRF` module (lib/bg_nerf/source/models/frequency_nerf.py:72-343)
on the render path used by `Graph.render` (lib/bg_nerf/source/models/renderer.py:532-627).

Same constructor arguments (`opt` tree), same parameter names (`mlp_feat.{0..7}.{weight,bias}`, `mlp_rgb.{0,1}.{weight,bias}`,
`progress`) and shapes - a reference `state_dict` loads as is - and the same methods:

    forward_samples(opt, center, ray, depth_samples, embedder_pts, embedder_view, mode)  -> rgb_samples, density_samples
    forward(opt, points_3D_samples, ray, embedder_pts, embedder_view, mode)
    composite(opt, ray, pred_dict, depth_samples)  -> rgb, rgb_var, depth, depth_var, opacity, weights, all_cumulated

Everything numerical runs in the HIP kernels of csrc/pp_nerf.hip through the C ABI (pp_nerf_fwd / pp_nerf_bwd /
pp_nerf_composite_fwd / pp_nerf_composite_bwd; pp_nerf_infer for the forward-only whole-view path, SceneRenderer.render_view /
render_rays); there is no eager fallback.  The parameters are views into ONE packed
device buffer in the layout the kernels read (`pp_nerf_layout`), so nothing is repacked per step and the whole network is a
single flat tensor for the fused Adam kernel (SceneEngine below).

Supported architecture = the reference default (lib/bg_nerf/train_settings/default_config.py:90-105) that every shipped
PoseProbe configuration uses; anything else raises NotImplementedError rather than silently taking another path.
"""
import math
import weakref

import torch

from . import ops


class Options(dict):
    """Attribute-style settings tree (stands in for the reference's easydict)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v


def default_options(barf_c2f=(0.4, 0.7), sample_intvs=128, white_bg=False):
    """The settings the render path reads, at the values PoseProbe trains with (lib/bg_nerf/train_settings/default_config.py
    :90-120, joint_pose_nerf_training/dtu/sparf.py)."""
    posenc = Options(include_pi_in_posenc=True, add_raw_3D_points=True, add_raw_rays=True, log_sampling=True, L_3D=10, L_view=4)
    arch = Options(layers_feat=[None] + [256] * 8, layers_feat_fine=None, layers_rgb=[None, 128, 3], skip=[4], posenc=posenc,
                   density_activ='softplus', tf_init=True)
    nerf = Options(view_dep=True, density_noise_reg=False, setbg_opaque=white_bg, sample_intvs=sample_intvs,
                   sample_stratified=True, fine_sampling=False, sample_intvs_fine=128, rand_rays=1024,
                   depth=Options(param='metric', range=[1, 0]))
    return Options(arch=arch, nerf=nerf, barf_c2f=list(barf_c2f) if barf_c2f else None, mask_img=False,
                   camera=Options(ndc=False), huber_loss_for_photometric=True)


def sparf_dtu_options(barf_c2f=(0.4, 0.7), sample_intvs=128, white_bg=False, max_iter=60000):
    """default_options plus the loss settings of the reference's DTU configuration (joint_pose_nerf_training/dtu/sparf.py:40-74)
    and the correspondence loss's own defaults (corres_loss.py:37-46): photometric + correspondence (+ depth consistency,
    which contributes nothing to the gradient in the reference - see trainer.loss_terms), weights 10^0 / 10^-2 / 10^-3, the
    correspondence weight halved every 5000 iterations from iteration 0 on, hierarchical sampling from 0.3 * max_iter on."""
    opt = default_options(barf_c2f=barf_c2f, sample_intvs=sample_intvs, white_bg=white_bg)
    opt.nerf.fine_sampling = True
    opt.nerf.ratio_start_fine_sampling_at_x = 0.3
    opt.update(max_iter=max_iter, loss_type='photometric_and_corres_and_depth_cons',
               loss_weight=Options(equalize_losses=False, parametrization='exp', render=0, corres=-2., depth_cons=-3),
               start_iter=Options(photometric=0, corres=0, depth_cons=0),
               gradually_decrease_corres_weight=True, ratio_start_decrease_corres_weight=0., iter_start_decrease_corres_weight=0,
               corres_weight_reduct_at_x_iter=5000, diff_loss_type='huber', renderrepro_do_pixel_reprojection_check=False,
               renderrepro_do_depth_reprojection_check=False, renderrepro_pixel_reprojection_thresh=10.,
               renderrepro_depth_reprojection_thresh=0.1)
    return opt


def stratified_depths(opt, rand, depth_range):
    """Stratified depths from uniform draws (renderer.py:665-700): rand [..., S, 1] (the reference's sample layout; a trailing
    axis of 1 is read as that) or [..., S], fresh or replayed, on the device the depths are wanted on.  Sample i of a ray lies
    in the i-th of S equal bins of depth_range, then goes through the opt.nerf.depth.param map."""
    column = rand.dim() > 1 and rand.shape[-1] == 1
    S = rand.shape[-2] if column else rand.shape[-1]
    steps = torch.arange(S, device=rand.device).float()
    depth = (rand + (steps[:, None] if column else steps)) / S * (depth_range[1] - depth_range[0]) + depth_range[0]
    return {'metric': depth, 'inverse': 1 / (depth + 1e-8)}[opt.nerf.depth.param]


def sample_depth(opt, batch_size, num_rays, n_samples, depth_range, mode=None, device='cuda', generator=None):
    """Stratified depth samples [B, num_rays, n_samples, 1] (renderer.py:665-700)."""
    if opt.nerf.sample_stratified and mode not in ('val', 'eval', 'test'):
        rand = torch.rand(batch_size, num_rays, n_samples, 1, device=device, generator=generator)
    else:
        rand = 0.5 * torch.ones(batch_size, num_rays, n_samples, 1, device=device)
    return stratified_depths(opt, rand, depth_range)


def sample_depth_from_pdf(weights, n_samples_coarse, n_samples_fine, depth_range, det, generator=None, grid=None):
    """Inverse-transform sampling from the coarse weights (renderer.py:702-738); weights [B, R, N] -> [B, R, Nf, 1].
    `grid` [Nf + 1] replays a recorded draw of the (shared across rays) uniform grid; a grid [R, Nf + 1] gives every ray its
    own (rays of separate render calls that share one pass)."""
    depth_min, depth_max = depth_range
    dev = weights.device
    pdf = weights / (weights.sum(dim=-1, keepdim=True) + 1e-6)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), pdf.cumsum(dim=-1)], dim=-1)
    if grid is not None:
        grid = grid.to(dev)
    elif det:
        grid = torch.linspace(0, 1, n_samples_fine + 1, device=dev)
    else:
        grid = torch.rand(n_samples_fine + 1, generator=generator).to(dev)
    if grid.dim() == 2:
        unif = (0.5 * (grid[:, :-1] + grid[:, 1:])).expand(*cdf.shape[:-1], n_samples_fine).contiguous()
    else:
        unif = (0.5 * (grid[:-1] + grid[1:])).repeat(*cdf.shape[:-1], 1)
    idx = torch.searchsorted(cdf, unif, right=True)
    bins = torch.linspace(depth_min, depth_max, n_samples_coarse + 1, device=dev).repeat(*cdf.shape[:-1], 1)
    lo, hi = (idx - 1).clamp(min=0), idx.clamp(max=n_samples_coarse)
    d_lo, d_hi = bins.gather(2, lo), bins.gather(2, hi)
    c_lo, c_hi = cdf.gather(2, lo), cdf.gather(2, hi)
    t = (unif - c_lo) / (c_hi - c_lo + 1e-8)
    return (d_lo + t * (d_hi - d_lo))[..., None]


class _LinearParams(torch.nn.Module):
    """Holds `weight` / `bias` (views into the packed block) under the reference's `torch.nn.Linear` names."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = torch.nn.Parameter(weight)
        self.bias = torch.nn.Parameter(bias)


class _Workspace:
    """Per-shape buffers that no pending backward depends on: the backward pass's scratch (used only inside one pp_nerf_bwd
    call), the device-side sample count, and an activation block for passes that nobody will differentiate through autograd
    (no_grad forwards, SceneEngine's own forward / backward pairs).  A forward pass that autograd may differentiate owns its
    activation block (see _NerfSamples): any number of them may be pending at the same shape, as in the reference."""

    def __init__(self, R, S, dev):
        M = R * S
        self.acts_floats, self.scratch_floats = ops.nerf_workspace(M, R)
        self.R, self.S, self.dev = R, S, dev
        self._acts = self._scratch = None
        self.count = torch.tensor([M], dtype=torch.int32, device=dev)
        self.scene_pass = None                # the ScenePass of this shape, made by NeRF.scene_pass and evicted with this

    @property
    def acts(self):
        if self._acts is None:
            self._acts = torch.empty(self.acts_floats, dtype=torch.float32, device=self.dev)
        return self._acts

    @property
    def scratch(self):                        # (a forward-only user never asks for it)
        if self._scratch is None:
            self._scratch = torch.zeros(self.scratch_floats, dtype=torch.float32, device=self.dev)
        return self._scratch

    def new_acts(self):
        return torch.empty(self.acts_floats, dtype=torch.float32, device=self.dev)


class ScenePass:
    """One forward / backward pair of one network at one (R rays x S samples) shape, without autograd: the sample outputs
    (rgb_s, dens), the compositing outputs (rgb, d, op, w, cum, rv, dv) and - from the first backward on - the sample and ray
    gradients (g_rgb_s, g_dens, g_ray_c, g_center, g_ray) and zero_r, as attributes.  One per network and shape
    (NeRF.scene_pass), shared by everything that runs such pairs on the network - SceneEngine, pose_refine.PoseRefiner, the
    forward-only SceneRenderer.render_view / render_rays - and overwritten by every call: a pair is forward, then backward,
    with nothing of the same network and shape in between.  The loss gradients g_rgb / g_depth belong to the caller."""

    def __init__(self, net, ws):
        self.net, self.ws = weakref.proxy(net), weakref.proxy(ws)          # both outlive the pass they hold: no cycle
        R, S = ws.R, ws.S
        f = dict(dtype=torch.float32, device=ws.dev)
        self.R, self.S, self._f = R, S, f
        self.rgb_s, self.dens = torch.empty(R * S, 3, **f), torch.empty(R * S, **f)
        self.rgb, self.w = torch.empty(R, 3, **f), torch.empty(R, S, **f)
        self.d, self.op, self.cum, self.rv, self.dv = (torch.empty(R, **f) for _ in range(5))
        self.g_rgb_s = self._work = None

    def forward(self, center, ray, depth, keep_acts=True):
        """center, ray [R,3], depth [R,S], contiguous fp32: pp_nerf_fwd into the shape's shared activation block and
        pp_nerf_composite_fwd.  keep_acts=False (no backward follows): pp_nerf_infer on its own workspace - 224 floats per
        sample against the 2337 + 256 mask bytes of the activation block - where the network's context selects the route it
        has.  -> self"""
        net, ws, R, S = self.net, self.ws, self.R, self.S
        if not keep_acts and net.infer_route():
            if self._work is None:
                self._work = torch.empty(ops.nerf_infer_workspace(R * S, R), **self._f)
            ops.nerf_infer(net.flat, center, ray, depth, net.band_weights(), ws.count, R, S, self._work, self.rgb_s, self.dens,
                           net.ctx)
        else:
            ops.nerf_fwd(net.flat, center, ray, depth, net.band_weights(), ws.count, R, S, ws.acts, self.rgb_s, self.dens, net.ctx)
        ops.nerf_composite_fwd(self.rgb_s, self.dens, depth, ray, R, S, net.white_bg, self.rgb, self.d, self.op, self.w, self.cum,
                               self.rv, self.dv)
        return self

    def _composite_bwd(self, ray, depth, g_rgb, g_depth):
        if self.g_rgb_s is None:
            R, S, f = self.R, self.S, self._f
            self.g_rgb_s, self.g_dens = torch.empty(R * S, 3, **f), torch.empty(R * S, **f)
            self.g_ray_c, self.g_center, self.g_ray = (torch.empty(R, 3, **f) for _ in range(3))
            self.zero_r = torch.zeros(R, **f)
        ops.nerf_composite_bwd(self.rgb_s, self.dens, depth, ray, self.w, self.R, self.S, self.net.white_bg, g_rgb,
                               self.zero_r if g_depth is None else g_depth, self.zero_r, None, self.g_rgb_s, self.g_dens,
                               self.g_ray_c)

    def backward(self, ray, depth, g_rgb, g_depth, grad_block):
        """Backward of the last forward(): g_rgb [R,3], g_depth [R] (None: zero) = d loss / d (rgb, d) -> g_center, g_ray [R,3];
        the parameter gradients are accumulated into grad_block."""
        net, ws = self.net, self.ws
        self._composite_bwd(ray, depth, g_rgb, g_depth)
        ops.nerf_bwd(net.flat, ray, depth, ws.count, self.R, self.S, ws.acts, self.rgb_s, self.g_rgb_s, self.g_dens, ws.scratch,
                     grad_block, self.g_center, self.g_ray, net.ctx)
        return self.g_center, self.g_ray + self.g_ray_c

    def backward_input(self, ray, depth, g_rgb, g_depth=None):
        """backward() that forms no parameter gradient (pp_nerf_bwd_input): the network stays frozen."""
        net, ws = self.net, self.ws
        self._composite_bwd(ray, depth, g_rgb, g_depth)
        ops.nerf_bwd_input(net.flat, ray, depth, ws.count, self.R, self.S, ws.acts, self.rgb_s, self.g_rgb_s, self.g_dens,
                           ws.scratch, self.g_center, self.g_ray, net.ctx)
        return self.g_center, self.g_ray + self.g_ray_c


def plan_chunks(n_rays, chunk_rays):
    """[(first ray, rays)] of a walk over n_rays rays in chunks of chunk_rays; the last chunk may be ragged."""
    n_rays, chunk_rays = int(n_rays), int(chunk_rays)
    if chunk_rays < 1:
        raise ValueError(f'chunk_rays = {chunk_rays}: at least one ray per chunk')
    if n_rays < 1:
        raise ValueError(f'n_rays = {n_rays}: nothing to render')
    return [(c, min(chunk_rays, n_rays - c)) for c in range(0, n_rays, chunk_rays)]


VIEW_MODES = ('val', 'eval', 'test')
VIEW_KEYS = ('rgb', 'rgb_var', 'depth', 'depth_var', 'opacity', 'all_cumulated')


def _check_view_args(mode, n_rays, chunk_rays):
    if mode not in VIEW_MODES:
        raise ValueError(f"mode {mode!r}: render_view / render_rays are forward-only and deterministic, mode must be one of "
                         f"{VIEW_MODES} (render / render_by_slices serve the stochastic ones)")
    return plan_chunks(n_rays, chunk_rays)


class _NerfSamples(torch.autograd.Function):
    """center[R,3], ray[R,3], depth[R,S] -> rgb_samples[R*S,3], density_samples[R*S]."""

    @staticmethod
    def forward(ctx, net, center, ray, depth, *params):
        R, S = depth.shape
        ws = net._workspace(R, S)
        f = dict(dtype=torch.float32, device=depth.device)
        center, ray, depth = center.contiguous().float(), ray.contiguous().float(), depth.contiguous().float()
        rgb_s, dens = torch.empty(R * S, 3, **f), torch.empty(R * S, **f)
        # a pass that may be differentiated keeps its own activations until its backward has run (the caching allocator
        # recycles the block afterwards); anything else shares the per-shape block
        acts = ws.new_acts() if any(ctx.needs_input_grad) else ws.acts
        ops.nerf_fwd(net.flat, center, ray, depth, net.band_weights(), ws.count, R, S, acts, rgb_s, dens, net.ctx)
        ctx.net, ctx.ws, ctx.acts = net, ws, acts
        ctx.save_for_backward(ray, depth, rgb_s)
        return rgb_s, dens

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb_s, g_dens):
        net, ws, acts = ctx.net, ctx.ws, ctx.acts
        ray, depth, rgb_s = ctx.saved_tensors
        ctx.acts = None                                            # once_differentiable: the block is free after this call
        R, S = depth.shape
        f = dict(dtype=torch.float32, device=depth.device)
        pgrad = torch.zeros_like(net.flat)
        g_center, g_ray = torch.empty(R, 3, **f), torch.empty(R, 3, **f)
        ops.nerf_bwd(net.flat, ray, depth, ws.count, R, S, acts, rgb_s, g_rgb_s.contiguous().float(),
                     g_dens.contiguous().float(), ws.scratch, pgrad, g_center, g_ray, net.ctx)
        return (None, g_center, g_ray, None, *net._views(pgrad))


class _Composite(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgb_s, dens, depth, ray, white_bg):
        R, S = depth.shape
        f = dict(dtype=torch.float32, device=depth.device)
        rgb_s, dens, depth, ray = (t.contiguous().float() for t in (rgb_s, dens, depth, ray))
        rgb, d, op, w = torch.empty(R, 3, **f), torch.empty(R, **f), torch.empty(R, **f), torch.empty(R, S, **f)
        cum, rv, dv = torch.empty(R, **f), torch.empty(R, **f), torch.empty(R, **f)
        ops.nerf_composite_fwd(rgb_s, dens, depth, ray, R, S, white_bg, rgb, d, op, w, cum, rv, dv)
        ctx.save_for_backward(rgb_s, dens, depth, ray, w)
        ctx.white_bg = white_bg
        ctx.mark_non_differentiable(cum, rv, dv)
        return rgb, d, op, w.clone(), cum, rv, dv

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_rgb, g_d, g_op, g_w, *_):
        rgb_s, dens, depth, ray, w = ctx.saved_tensors
        R, S = depth.shape
        f = dict(dtype=torch.float32, device=depth.device)
        g_rgb_s, g_dens, g_ray = torch.empty(R * S, 3, **f), torch.empty(R * S, **f), torch.empty(R, 3, **f)
        ops.nerf_composite_bwd(rgb_s, dens, depth, ray, w, R, S, ctx.white_bg, g_rgb.contiguous(), g_d.contiguous(),
                               g_op.contiguous(), g_w.contiguous(), g_rgb_s, g_dens, g_ray)
        return g_rgb_s, g_dens, None, g_ray, None


class NeRF(torch.nn.Module):
    """MLP network corresponding to NeRF (frequency_nerf.py:72)."""

    L_3D, L_VIEW = 10, 4

    def __init__(self, opt, is_fine_network=False, device='cuda', options=None):
        """options: {name: value} of a private pp_context for this network's kernels (e.g. {'nerf_split': 0}: every product on
        the fp32 MFMA instructions); None = the host's default context."""
        super().__init__()
        self.opt = opt
        self.ctx = ops.Context(**options) if options else None
        self._check_supported(opt, is_fine_network)
        off = ops.nerf_layout()
        self._off = off
        dev = torch.device(device)
        self.flat = torch.zeros(off[22], dtype=torch.float32, device=dev)
        w, b = self._views(self.flat, split=True)
        self.mlp_feat = torch.nn.ModuleList([_LinearParams(w[i], b[i]) for i in range(8)])
        self.mlp_rgb = torch.nn.ModuleList([_LinearParams(w[8 + i], b[8 + i]) for i in range(2)])
        if opt.arch.tf_init:
            self.initialize()
        # a Parameter so that it is checkpointed, as in the reference (frequency_nerf.py:79-85)
        self.progress = torch.nn.Parameter(torch.tensor(1. if opt.barf_c2f is None else 0., device=dev))
        self._ws = {}

    @staticmethod
    def _check_supported(opt, is_fine_network):
        a, p = opt.arch, opt.arch.posenc
        layers = a.layers_feat_fine if is_fine_network and a.layers_feat_fine is not None else a.layers_feat
        ok = (list(layers[1:]) == [256] * 8 and list(a.layers_rgb[1:]) == [128, 3] and list(a.skip) == [4] and p.L_3D == 10
              and p.L_view == 4 and p.add_raw_3D_points and p.add_raw_rays and p.log_sampling and p.include_pi_in_posenc
              and a.density_activ == 'softplus' and opt.nerf.view_dep and not opt.nerf.density_noise_reg)
        if not ok:
            raise NotImplementedError('bg_nerf: only the reference default architecture (8 x 256, skip [4], L_3D = 10, '
                                      'L_view = 4 with raw coordinates, softplus density, view dependent colour, no density '
                                      'noise) has HIP kernels')

    def _views(self, flat, split=False):
        """Per-parameter views of a packed block in registration order (mlp_feat.i.weight, .bias, ..., mlp_rgb.i.*)."""
        o = self._off
        w, b = [], []
        for l, k in enumerate((64, 256, 256, 256, 320, 256, 256)):
            used = {0: 63, 4: 319}.get(l, k)
            w.append(flat[o[2 * l]:o[2 * l] + 256 * k].view(256, k)[:, :used])
            b.append(flat[o[2 * l + 1]:o[2 * l + 1] + 256])
        w.append(flat[o[16]:o[16] + 257 * 256].view(257, 256))          # density row + 256 feature rows
        b.append(flat[o[17]:o[17] + 257])
        w.append(flat[o[18]:o[18] + 128 * 288].view(128, 288)[:, :283])
        b.append(flat[o[19]:o[19] + 128])
        w.append(flat[o[20]:o[20] + 3 * 128].view(3, 128))
        b.append(flat[o[21]:o[21] + 3])
        if split:
            return w, b
        return [t for pair in zip(w, b) for t in pair]

    def _apply(self, fn, *a, **k):
        probe = fn(torch.empty(0, device=self.flat.device))
        if probe.device != self.flat.device or probe.dtype != torch.float32:
            raise RuntimeError('bg_nerf.NeRF lives in one packed fp32 device buffer: construct it with device=... instead of '
                               'moving / casting it')
        return self

    def state_dict(self, *args, **kwargs):
        """Compact copies under the reference's names: the parameters are views into the packed block, and serialising a view
        would write the whole 2 MB block once per tensor."""
        sd = super().state_dict(*args, **kwargs)
        for k in list(sd.keys()):
            sd[k] = sd[k].clone()
        return sd

    def initialize(self):
        """TensorFlow-style Xavier initialisation (frequency_nerf.py:128-148)."""
        gain = torch.nn.init.calculate_gain('relu')
        with torch.no_grad():
            for li, lin in enumerate(self.mlp_feat):
                if li == len(self.mlp_feat) - 1:
                    torch.nn.init.xavier_uniform_(lin.weight[:1])
                    torch.nn.init.xavier_uniform_(lin.weight[1:], gain=gain)
                else:
                    torch.nn.init.xavier_uniform_(lin.weight, gain=gain)
                lin.bias.zero_()
            torch.nn.init.xavier_uniform_(self.mlp_rgb[0].weight, gain=gain)
            torch.nn.init.xavier_uniform_(self.mlp_rgb[1].weight)
            self.mlp_rgb[0].bias.zero_(), self.mlp_rgb[1].bias.zero_()

    # ------------------------------------------------------------------------------------------------------------
    def band_weights(self):
        """Device tensor [14]: coarse-to-fine weights of the 10 point bands and the 4 view bands (frequency_nerf.py:255-262),
        computed on the device from `progress` (the trainer updates it with in-place fills on `.data`, which no version
        counter sees) so the schedule never forces a host synchronisation; same elementwise op order as the reference."""
        dev = self.flat.device
        if self.opt.barf_c2f is None:
            if getattr(self, '_band_ones', None) is None:
                self._band_ones = torch.ones(14, dtype=torch.float32, device=dev)
            return self._band_ones
        start, end = self.opt.barf_c2f
        if dev.type == 'cuda':
            # one launch (pp_nerf_band_weights); a ring of outputs, because a pending autograd backward may still hold the
            # weights of an earlier forward while `progress` moves on
            if getattr(self, '_band_ring', None) is None:
                self._band_ring, self._band_i = torch.empty(16, 14, dtype=torch.float32, device=dev), 0
            out = self._band_ring[self._band_i]
            self._band_i = (self._band_i + 1) % 16
            ops.nerf_band_weights(self.progress.data, float(start), float(end), self.L_3D, self.L_VIEW, out)
            return out
        if getattr(self, '_band_consts', None) is None:
            L = torch.tensor([float(self.L_3D)] * self.L_3D + [float(self.L_VIEW)] * self.L_VIEW, device=dev)
            k = torch.tensor(list(range(self.L_3D)) + list(range(self.L_VIEW)), dtype=torch.float32, device=dev)
            self._band_consts = (L, k)
        L, k = self._band_consts
        alpha = (self.progress.data - start) / (end - start) * L
        return (1 - (alpha - k).clamp_(min=0, max=1).mul_(math.pi).cos_()) / 2

    def _workspace(self, R, S):
        ws = self._ws.get((R, S))
        if ws is None:
            if len(self._ws) >= 4:
                self._ws.clear()
            ws = self._ws[(R, S)] = _Workspace(R, S, self.flat.device)
        return ws

    def infer_route(self):
        """True when this network's context selects the route pp_nerf_infer has (the fused one: nerf_split = 1, nerf_chain = 3,
        the defaults); otherwise forward-only passes go through pp_nerf_fwd and the shared block."""
        from . import _lib
        c = self.ctx if self.ctx is not None else _lib.default_context()
        return c.get('nerf_split') == 1 and c.get('nerf_chain') == 3

    @property
    def white_bg(self):
        """Composite onto a white background (frequency_nerf.py:337)."""
        return bool(self.opt.nerf.setbg_opaque or self.opt.mask_img)

    def scene_pass(self, R, S):
        """The ScenePass of this network at R rays x S samples, cached on (and evicted with) the shape's workspace."""
        ws = self._workspace(R, S)
        if ws.scene_pass is None:
            ws.scene_pass = ScenePass(self, ws)
        return ws.scene_pass

    @torch.no_grad()
    def infer_composite(self, opt, center, ray, depth):
        """center, ray [R,3], depth [R,S], contiguous fp32 -> the ScenePass of the shape, holding rgb_s, dens and the
        compositing outputs of this call (overwritten by the next pass of the same shape).  Forward only: pp_nerf_infer (or, on
        another route, pp_nerf_fwd into the shared activation block) and pp_nerf_composite_fwd."""
        return self.scene_pass(*depth.shape).forward(center, ray, depth, keep_acts=False)

    def _params(self):
        return [p for lin in list(self.mlp_feat) + list(self.mlp_rgb) for p in (lin.weight, lin.bias)]

    def forward_samples(self, opt, center, ray, depth_samples, embedder_pts=None, embedder_view=None, mode=None):
        """center, ray [B, N, 3]; depth_samples [B, N, S, 1] (frequency_nerf.py:268-288).  The embedders are accepted for
        signature compatibility; the encoding is part of the kernel."""
        B, N, S = depth_samples.shape[:3]
        rgb_s, dens = _NerfSamples.apply(self, center.reshape(B * N, 3), ray.reshape(B * N, 3),
                                         depth_samples.reshape(B * N, S), *self._params())
        return dict(rgb_samples=rgb_s.view(B, N, S, 3), density_samples=dens.view(B, N, S))

    def forward(self, opt, points_3D_samples, ray, embedder_pts=None, embedder_view=None, mode=None):
        """points_3D_samples [B, N, S, 3], ray [B, N, 3] (frequency_nerf.py:172-227): every point is a one-sample ray at
        depth 0 whose origin is the point itself."""
        B, N, S = points_3D_samples.shape[:3]
        pts = points_3D_samples.reshape(B * N * S, 3)
        rays = ray[:, :, None, :].expand(B, N, S, 3).reshape(B * N * S, 3)
        rgb_s, dens = _NerfSamples.apply(self, pts, rays, torch.zeros(B * N * S, 1, device=pts.device), *self._params())
        return dict(rgb_samples=rgb_s.view(B, N, S, 3), density_samples=dens.view(B, N, S))

    def composite(self, opt, ray, pred_dict, depth_samples):
        """Quadrature compositing (frequency_nerf.py:290-343); adds rgb, rgb_var, depth, depth_var, opacity, weights,
        all_cumulated to pred_dict.  depth_samples are treated as constants, as produced by the stratified sampler."""
        B, N, S = depth_samples.shape[:3]
        rgb, d, op, w, cum, rv, dv = _Composite.apply(pred_dict['rgb_samples'].reshape(B * N * S, 3),
                                                     pred_dict['density_samples'].reshape(B * N * S),
                                                     depth_samples.reshape(B * N, S), ray.reshape(B * N, 3), self.white_bg)
        pred_dict.update(rgb=rgb.view(B, N, 3), rgb_var=rv.view(B, N, 1), depth=d.view(B, N, 1), depth_var=dv.view(B, N, 1),
                         opacity=op.view(B, N, 1), weights=w.view(B, N, S, 1), all_cumulated=cum.view(B, N))
        return pred_dict


def _cam2world(X, pose_w2c):
    """camera -> world for points X [B, N, 3] under world-to-camera poses [B, 3, 4] (utils/camera.py:321-338)."""
    Rinv = pose_w2c[..., :3].transpose(-1, -2)
    c2w = torch.cat([Rinv, -Rinv @ pose_w2c[..., 3:]], dim=-1)
    return torch.cat([X, torch.ones_like(X[..., :1])], dim=-1) @ c2w.transpose(-1, -2)


def get_center_and_ray_at_pixels(pose_w2c, pixels, intr):
    """Camera centres and un-normalised ray directions of given pixels (utils/camera.py:384-416): pixels [N, 2] (shared by
    all images) or [B, N, 2]; differentiable w.r.t. the poses through a handful of per-ray torch ops."""
    B = len(pose_w2c)
    xy = pixels.unsqueeze(0).repeat(B, 1, 1) if pixels.dim() == 2 else pixels
    grid = torch.cat([xy, torch.ones_like(xy[..., :1])], dim=-1) @ intr.inverse().transpose(-1, -2)
    center = _cam2world(torch.zeros_like(grid), pose_w2c)
    return center, _cam2world(grid, pose_w2c) - center


def get_center_and_ray(pose_w2c, H, W, intr):
    """All H * W pixel centres (x + 0.5, y + 0.5), row-major (utils/camera.py:347-381)."""
    dev = pose_w2c.device
    Y, X = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev) + 0.5,
                          torch.arange(W, dtype=torch.float32, device=dev) + 0.5, indexing='ij')
    return get_center_and_ray_at_pixels(pose_w2c, torch.stack([X, Y], dim=-1).view(-1, 2), intr)


class SceneRenderer:
    """The render path of the reference's `Graph` (renderer.py:532-627): rays from poses, stratified coarse samples, coarse
    NeRF + compositing and - once `iter` has passed `ratio_start_fine_sampling_at_x * max_iter` - the fine NeRF on the union of
    the coarse samples and inverse-transform samples of the coarse weights.  Returns the same keys (`*_fine` for the second
    pass).  `rand` (optional) replays recorded uniform draws: [coarse [B, N, S, 1], fine grid [Nf + 1]]."""

    def __init__(self, opt, device='cuda', nerf=None, nerf_fine=None):
        """nerf (and nerf_fine): render with these existing networks instead of building new ones (their device is used)."""
        if nerf is not None:
            self.opt, self.device, self.nerf, self.nerf_fine = opt, nerf.flat.device, nerf, nerf_fine
            return
        self.opt, self.device = opt, torch.device(device)
        self.nerf = NeRF(opt, device=device)
        self.nerf_fine = NeRF(opt, is_fine_network=True, device=device) if opt.nerf.fine_sampling else None

    def render(self, opt, pose, H, W, intr, pixels=None, ray_idx=None, depth_range=None, iter=None, mode=None, rand=None):
        B = len(pose)
        if pixels is not None:
            center, ray = get_center_and_ray_at_pixels(pose, pixels, intr)
        else:
            center, ray = get_center_and_ray(pose, H, W, intr)
            if ray_idx is not None:
                if ray_idx.dim() == 2 and ray_idx.shape[0] == B:
                    bi = torch.arange(B, device=ray_idx.device)[:, None]
                    center, ray = center[bi, ray_idx.long()], ray[bi, ray_idx.long()]
                else:
                    center, ray = center[:, ray_idx], ray[:, ray_idx]
        if opt.camera.ndc:
            raise NotImplementedError('bg_nerf: NDC rays are not used by any PoseProbe configuration')
        N, S = ray.shape[1], opt.nerf.sample_intvs
        pred = Options(origins=center, viewdirs=ray)
        if rand is not None:
            depth = stratified_depths(opt, rand[0].to(self.device), depth_range)
        else:
            depth = sample_depth(opt, B, N, S, depth_range, mode=mode, device=self.device)
        coarse = self.nerf.forward_samples(opt, center, ray, depth, mode=mode)
        coarse['t'] = depth
        pred.update(self.nerf.composite(opt, ray, coarse, depth))
        if self._fine_active(opt, iter):
            with torch.no_grad():
                det = mode not in ('train', 'test-optim') or not opt.nerf.sample_stratified
                grid = rand[1].to(self.device) if (rand is not None and not det) else None
                fine_t = sample_depth_from_pdf(pred['weights'][..., 0].detach(), S, opt.nerf.sample_intvs_fine, depth_range,
                                               det=det, grid=grid)
            depth = torch.cat([depth, fine_t], dim=2).sort(dim=2).values
            fine = self.nerf_fine.forward_samples(opt, center, ray, depth, mode=mode)
            fine['t'] = depth
            fine = self.nerf_fine.composite(opt, ray, fine, depth)
            pred.update({k + '_fine': v for k, v in fine.items()})
        return pred


    def render_up_to_maxdepth(self, opt, pose, H, W, intr, depth_max, depth_min, pixels, iter=None, mode=None):
        """Rendering with a different far bound per ray (renderer.py:742-878, sample_depth_diff_max_range_per_ray :880-909):
        depth_max [B, N]; deterministic samples depth_min + (i + 1) / S * (depth_max - depth_min); the fine network, when
        active, is evaluated on the SAME samples (only the accumulated transmittance is wanted from this pass)."""
        center, ray = get_center_and_ray_at_pixels(pose, pixels, intr)
        S = opt.nerf.sample_intvs
        steps = (1.0 + torch.arange(S, device=self.device).float())[None, None, :, None] / S
        depth = steps * (depth_max[..., None, None] - depth_min) + depth_min
        pred = Options(origins=center, viewdirs=ray)
        coarse = self.nerf.forward_samples(opt, center, ray, depth, mode=mode)
        coarse['t'] = depth
        pred.update(self.nerf.composite(opt, ray, coarse, depth))
        if self._fine_active(opt, iter):
            fine = self.nerf_fine.forward_samples(opt, center, ray, depth, mode=mode)
            fine['t'] = depth
            fine = self.nerf_fine.composite(opt, ray, fine, depth)
            pred.update({k + '_fine': v for k, v in fine.items()})
        return pred

    @torch.no_grad()
    def render_by_slices(self, opt, pose, H, W, intr, depth_range, iter=None, mode=None):
        """Full H x W images in slices of `opt.nerf.rand_rays` rays (renderer.py:629-663): per-ray outputs concatenated along
        the ray axis, `*_fine` keys when the fine pass is active."""
        keys = ['rgb', 'rgb_var', 'depth', 'depth_var', 'opacity', 'all_cumulated']
        parts = {}
        for c in range(0, H * W, opt.nerf.rand_rays):
            ray_idx = torch.arange(c, min(c + opt.nerf.rand_rays, H * W), device=self.device)
            ret = self.render(opt, pose, H, W, intr, ray_idx=ray_idx, depth_range=depth_range, iter=iter, mode=mode)
            for k in keys + [k + '_fine' for k in keys]:
                if k in ret:
                    parts.setdefault(k, []).append(ret[k])
        return Options({k: torch.cat(v, dim=1) for k, v in parts.items()})


    @staticmethod
    def _fine_active(opt, iter):
        """The fine pass runs when fine_sampling is set and `iter`, if both it and ratio_start_fine_sampling_at_x are given, has
        reached that share of max_iter (renderer.py:599-602)."""
        start = getattr(opt.nerf, 'ratio_start_fine_sampling_at_x', None)
        skip_fine = start is not None and iter is not None and iter < opt.max_iter * start
        return bool(opt.nerf.fine_sampling and not skip_fine)

    # ---- forward-only whole views ------------------------------------------------------------------------------------------
    def _render_chunk(self, opt, center, ray, depth_range, mode, fine, out, c):
        """One chunk - center, ray [B, n, 3], the rays c .. c + n - 1 of every pose - through render's sequence of functions on
        render's shapes (the B * n rays of a chunk are one pass, as in render), written into out[key][:, c:c + n]."""
        B, n = ray.shape[:2]
        S = opt.nerf.sample_intvs
        cen, r = center.reshape(B * n, 3).contiguous().float(), ray.reshape(B * n, 3).contiguous().float()
        depth = sample_depth(opt, B, n, S, depth_range, mode=mode, device=self.device)
        passes = [('', self.nerf.infer_composite(opt, cen, r, depth.reshape(B * n, S).contiguous().float()))]
        if fine:
            fine_t = sample_depth_from_pdf(passes[0][1].w.view(B, n, S), S, opt.nerf.sample_intvs_fine, depth_range, det=True)
            depth = torch.cat([depth, fine_t], dim=2).sort(dim=2).values
            passes.append(('_fine', self.nerf_fine.infer_composite(opt, cen, r, depth.reshape(B * n, -1).contiguous().float())))
        for sfx, b in passes:
            for k, t in (('rgb', b.rgb), ('rgb_var', b.rv), ('depth', b.d), ('depth_var', b.dv), ('opacity', b.op),
                         ('all_cumulated', b.cum)):
                o = out[k + sfx][:, c:c + n]
                o.copy_(t.view(o.shape))

    def _render_chunks(self, opt, center, ray, depth_range, mode, chunks, iter):
        if opt.camera.ndc:
            raise NotImplementedError('bg_nerf: NDC rays are not used by any PoseProbe configuration')
        B, N = ray.shape[:2]
        fine = self._fine_active(opt, iter)
        if fine and self.nerf_fine is None:
            raise ValueError('fine_sampling is active but this renderer has no fine network')
        f = dict(dtype=torch.float32, device=self.device)
        out = Options()
        for sfx in ('', '_fine') if fine else ('',):
            for k in VIEW_KEYS:
                out[k + sfx] = torch.empty((B, N) if k == 'all_cumulated' else (B, N, 3 if k == 'rgb' else 1), **f)
        for c, n in chunks:
            self._render_chunk(opt, center[:, c:c + n], ray[:, c:c + n], depth_range, mode, fine, out, c)
        return out

    @torch.no_grad()
    def render_rays(self, opt, center, ray, depth_range, mode='val', chunk_rays=8192, iter=None):
        """Forward-only render of given rays: center, ray [N,3] on the device -> render_by_slices' keys with B = 1 ([1,N,3],
        [1,N,1], all_cumulated [1,N]; `*_fine` when the fine pass is active).  Deterministic modes only (mid-point samples,
        det=True inverse-transform samples).  Per chunk of chunk_rays rays: sample_depth, pp_nerf_infer on the coarse network,
        pp_nerf_composite_fwd, sample_depth_from_pdf, concatenate + sort, pp_nerf_infer on the fine network,
        pp_nerf_composite_fwd - render's functions on render's per-ray inputs, with no activation kept (224 floats of workspace
        per sample instead of 2337 + 256 bytes), one workspace per chunk shape reused across chunks and calls, outputs written in
        place, no host read.  A network whose context selects another route than the default goes through pp_nerf_fwd and its
        shared activation block at the same chunking."""
        if center.dim() != 2 or center.shape != ray.shape or ray.shape[-1] != 3:
            raise ValueError('render_rays: center and ray must both be [N,3]')
        chunks = _check_view_args(mode, ray.shape[0], chunk_rays)
        return self._render_chunks(opt, center[None].to(self.device), ray[None].to(self.device), depth_range, mode, chunks, iter)

    @torch.no_grad()
    def render_view(self, opt, pose, H, W, intr, depth_range, mode='val', chunk_rays=8192, iter=None):
        """Forward-only render of whole H x W views: pose [1,3,4] or [B,3,4] (world to camera), intr [B,3,3] -> what
        render_by_slices returns (same keys, same shapes; bit-identical to it with opt.nerf.rand_rays = chunk_rays).  The rays are
        formed ONCE per call (render_by_slices forms all H * W of them again for every slice), then walked in chunks of
        chunk_rays rays per pose as in render_rays.  The default 8192 keeps the fine pass's workspace under 2 GiB at 256 samples
        per ray."""
        if pose.dim() != 3 or tuple(pose.shape[1:]) != (3, 4):
            raise ValueError('render_view: pose must be [B,3,4]')
        chunks = _check_view_args(mode, int(H) * int(W), chunk_rays)
        center, ray = get_center_and_ray(pose.to(self.device), H, W, intr.to(self.device))
        return self._render_chunks(opt, center, ray, depth_range, mode, chunks, iter)


def photometric_loss(rgb, image, huber=True):
    """Render loss of the branch (training/core/base_losses.py:151-156, :304-305)."""
    if huber:
        return torch.nn.functional.huber_loss(rgb, image, reduction='mean', delta=0.5) * 2.
    return torch.nn.functional.mse_loss(rgb, image)


class CorresRows:
    """The matched-pixel rows of one view pair for SceneEngine's union pass (corres_loss.py:140-222): pix_self, pix_other [M,2]
    (matcher pixel coordinates: rays through K^-1 [x, y, 1], no half-pixel offset), conf [M], the intrinsics K_self, K_other
    [3,3] and the CURRENT w2c_self, w2c_other [3,4] as device tensors (the kernel reads them; the host reads no pose), the loss
    weight (10^loss_weight.corres / gamma), the filters of `opt` (renderrepro_*, defaults of corres_loss.py:37-46), the
    photometric term's weight 10^loss_weight.render and, optionally, the replayed uniform grid of the tail's fine samples."""

    def __init__(self, pix_self, pix_other, conf, K_self, K_other, w2c_self, w2c_other, weight, opt=None, fine_grid=None,
                 photo_weight=1.0):
        if str(getattr(opt, 'diff_loss_type', 'huber')).lower() != 'huber':
            raise NotImplementedError('correspondence loss: only diff_loss_type = huber (the reference default) has a kernel')
        self.pix_self, self.pix_other, self.conf = pix_self.contiguous(), pix_other.contiguous(), conf.reshape(-1).contiguous()
        self.K_self, self.K_other, self.w2c_self, self.w2c_other = K_self, K_other, w2c_self, w2c_other
        self.weight, self.fine_grid, self.photo_weight = float(weight), fine_grid, float(photo_weight)
        self.pixel_check = bool(getattr(opt, 'renderrepro_do_pixel_reprojection_check', False))
        self.depth_check = bool(getattr(opt, 'renderrepro_do_depth_reprojection_check', False))
        self.pixel_thresh = float(getattr(opt, 'renderrepro_pixel_reprojection_thresh', 10.))
        self.depth_thresh = float(getattr(opt, 'renderrepro_depth_reprojection_thresh', 0.1))


class _NetState:
    """Gradient block and Adam moments of one packed network."""

    def __init__(self, net):
        self.net = net
        self.grad = torch.zeros_like(net.flat)
        self.m, self.v = torch.zeros_like(net.flat), torch.zeros_like(net.flat)
        self.seg_end = torch.tensor([net.flat.numel()], dtype=torch.int32, device=net.flat.device)
        self.steps = 0               # optimiser steps this network has taken (torch.optim.Adam keeps `step` per parameter)
        self.has_grad = False


class _LossRing:
    """256 slots for 0-dim losses that nobody reads back inside the step: a slot is rewritten 256 calls later."""

    def __init__(self, dev):
        self.slots, self.i = torch.zeros(256, dtype=torch.float32, device=dev), -1

    def next(self):
        self.i = (self.i + 1) % 256
        return self.slots[self.i]


class _LossGrads:
    """d loss / d (rgb, depth) of one of SceneEngine's passes at R rows, and the ring of its photometric losses.  A call with Rp
    photometric rows needs g_rgb [R,3] zero on the matched tail [Rp:] and g_depth [R] zero on the prefix [:Rp].  The loss
    kernels overwrite the other rows - huber all of g_rgb[:Rp], pp_nerf_corres_loss all of g_depth[Rp:] - and nothing else
    writes either buffer, so after a call both hold exactly that and `Rp` records the split; a call with another split zeroes
    its two ranges before the kernels run.  g_rgb is made for the first call's split (zeros if that call has a tail).  g_depth
    exists from the first call with matched rows on (all zero then: right for every split); a call without them gets None = the
    pass's own zeros."""

    def __init__(self, R, Rp, dev):
        self.R, self.Rp = R, Rp
        self.g_rgb, self.g_depth = (torch.empty if Rp == R else torch.zeros)(R, 3, dtype=torch.float32, device=dev), None
        self.losses = _LossRing(dev)

    def split(self, Rp, matched):
        """-> g_rgb, g_depth (None unless `matched`) ready for a call with Rp photometric rows."""
        if Rp != self.Rp:
            self.g_rgb[Rp:].zero_()
            if self.g_depth is not None:
                self.g_depth[:Rp].zero_()
            self.Rp = Rp
        if matched and self.g_depth is None:
            self.g_depth = torch.zeros(self.R, dtype=torch.float32, device=self.g_rgb.device)
        return self.g_rgb, self.g_depth if matched else None


class SceneEngine:
    """One optimisation step of the scene branch without autograd bookkeeping: forward, photometric loss, backward and one
    fused Adam update per packed parameter block (renderer.py:420-423 train_iteration + the optimiser step of
    lib/recon_scene.py:765).  With `net_fine` and `fine=True` the step is the reference's hierarchical one
    (renderer.py:586-611): the fine network runs on the union of the coarse samples and inverse-transform samples of the
    coarse weights, `loss = huber(rgb) + huber(rgb_fine)` (base_losses.py:304-307), both networks receive gradients.
    Ray gradients (sum over the passes) are returned for the caller's pose chain.

    deterministic=True: bit-reproducible step.  The one order-dependent sum of the kernels - the float-atomic flush of the nine
    weight-gradient products per pass - goes through per-work-group slots of a workspace and a reduction in a fixed order
    (ops.nerf_ordered_attach; 34 MB, allocated here once, shared by both networks), and the fine phase draws its samples with
    ops.nerf_sample_pdf (weight sum, cdf, search, interpolation and merge in one kernel with fixed orders) instead of torch's
    sum / cumsum, whose order on the device is not promised.  Each network gets a private context (the host's default context's
    values) if it has none; the workspace stays attached to the networks' contexts.  GUARANTEE: for a fixed build, fixed option
    values, fixed shapes and the same device model, identical inputs (state, center, ray, depth, image, replayed fine_grid,
    the same correspondence rows) give bit-identical flat, m, v of both networks and bit-identical returned gradients, in the
    coarse phase, the hierarchical phase and both with the correspondence term.  Only the split-precision kernels have the
    ordered flush: a network with nerf_split = 0 is refused with ValueError.  Not covered: SceneRenderer's autograd route, and
    multi-rank runs.  Off (default): nothing changes - same kernels, same launches, no context, no workspace."""

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, net_fine=None, deterministic=False):
        self.net, self.net_fine = net, net_fine
        self.deterministic = bool(deterministic)
        self._ordered_work = None
        if self.deterministic:
            from . import _lib
            nets = [net] + ([net_fine] if net_fine is not None else [])
            for n in nets:
                if (n.ctx.get('nerf_split') if n.ctx is not None else _lib.default_context().get('nerf_split')) != 1:
                    raise ValueError('deterministic=True with nerf_split = 0: the fp32-instruction weight-gradient kernel has no '
                                     'ordered gradient flush (it keeps float atomics)')
            work = next((n._ordered_work for n in nets if getattr(n, '_ordered_work', None) is not None), None)
            if work is None:
                work = torch.empty(ops.nerf_ordered_workspace(), dtype=torch.uint8, device=net.flat.device)
            self._ordered_work = work
            for n in nets:
                if n.ctx is None:
                    n.ctx = ops.Context(**_lib.default_context().options())
                ops.nerf_ordered_attach(n.ctx, work)
                n._ordered_work = work            # the context holds the address: the network keeps the buffer alive with it
        self.lr, self.betas, self.eps = lr, betas, eps
        self.states = [_NetState(net)] + ([_NetState(net_fine)] if net_fine is not None else [])
        self.grad, self.m, self.v = self.states[0].grad, self.states[0].m, self.states[0].v
        self.step_count = 0
        self.seg_lr = torch.tensor([lr], dtype=torch.float32, device=net.flat.device)
        self._loss_grads = {}                 # (pass, rows) -> _LossGrads
        self._corres = None                   # (loss ring, g_w2c [2,3,4]) of the correspondence term, from its first use on

    def forward_backward(self, center, ray, depth, image, fine=False, depth_range=None, fine_grid=None, corres=None):
        """center, ray [R,3]; depth [R,S]; image [Rp,3] -> (loss, g_center, g_ray); parameter gradients are accumulated into the
        networks' gradient blocks, which optimizer_step() consumes and re-zeroes.  fine=True adds the second pass
        (`depth_range` required; `fine_grid` [Nf + 1] replays the sampler's uniform draw).
        corres (CorresRows): the union pass - center / ray / depth hold R = Rp + 2M rows, image the Rp photometric rows, and the
        last 2M rows are the matched pixels of one view pair [self M | other M], in the same launches as the photometric rows
        (the reference renders them in two calls, renderer.py:420-423 and corres_loss.py:178-183).  Without it Rp = R.
        One order for every step: the forward of every pass (coarse, then fine on depths drawn from the coarse weights), then
        the losses - 2 * huber(delta = 0.5, mean) on the photometric prefix of every pass, pp_nerf_corres_loss on the tail,
        which needs the rendered depths of all passes - then the backward of every pass with g_rgb zero on the tail and g_depth
        zero on the prefix (_LossGrads).  Every loss lands in a ring slot (the returned 0-dim tensors are rewritten 256 calls
        later: read them - .item() / copy - before that).  With corres also sets last_terms (photometric, correspondence
        loss) and last_g_w2c [2,3,4] (the correspondence loss's direct pose gradient, overwritten next call)."""
        R, Rp = depth.shape[0], image.shape[0]
        M = 0 if corres is None else corres.pix_self.shape[0]
        if R != Rp + 2 * M:
            raise ValueError(f'SceneEngine: union pass of {R} rows, expected {Rp} photometric + 2 x {M} matched rows')
        if fine and (self.net_fine is None or depth_range is None):
            raise ValueError('SceneEngine: fine=True needs net_fine and depth_range')
        passes = [(self.states[0], self.net.scene_pass(*depth.shape).forward(center, ray, depth), depth)]
        if fine:
            depth_f = self._fine_depths(passes[0][1].w, depth, depth_range, fine_grid, Rp, corres)
            passes.append((self.states[1], self.net_fine.scene_pass(*depth_f.shape).forward(center, ray, depth_f), depth_f))
        image = image.contiguous()
        grads, loss = [], None
        for k, (st, p, dep) in enumerate(passes):
            lg = self._loss_grads.get((k, R))
            if lg is None:
                if len(self._loss_grads) >= 8:
                    self._loss_grads.clear()
                lg = self._loss_grads[(k, R)] = _LossGrads(R, Rp, depth.device)
            grads.append(lg.split(Rp, corres is not None))
            l = lg.losses.next()
            ops.nerf_huber_loss(p.rgb[:Rp], image, 0.5, 2.0 if corres is None else 2.0 * corres.photo_weight, l, lg.g_rgb[:Rp])
            loss = l if loss is None else loss + l
        if corres is not None:
            if self._corres is None:
                self._corres = _LossRing(depth.device), torch.zeros(2, 3, 4, dtype=torch.float32, device=depth.device)
            loss_corr, g_w2c = self._corres[0].next(), self._corres[1]
            ops.nerf_corres_loss(passes[0][1].d[Rp:], passes[1][1].d[Rp:] if fine else None, corres.pix_self, corres.pix_other,
                                 corres.conf, corres.K_self, corres.K_other, corres.w2c_self, corres.w2c_other, corres.pixel_check,
                                 corres.pixel_thresh, corres.depth_check, corres.depth_thresh, corres.weight, loss_corr,
                                 grads[0][1][Rp:], grads[1][1][Rp:] if fine else None, g_w2c)
            self.last_terms, self.last_g_w2c = dict(photometric=loss, corres=loss_corr), g_w2c
            loss = loss + loss_corr
        g_center = g_ray = None
        for (st, p, dep), (g_rgb, g_depth) in zip(passes, grads):
            gc, gr = p.backward(ray, dep, g_rgb, g_depth, st.grad)
            st.has_grad = True
            g_center, g_ray = (gc, gr) if g_center is None else (g_center + gc, g_ray + gr)
        return loss, g_center, g_ray

    def _fine_depths(self, w, depth, depth_range, fine_grid, Rp, corres):
        """The fine pass's sorted [R, S + Nf] depths: the coarse depths merged with Nf inverse-transform samples of the coarse
        weights w [R, S] on a uniform grid - replayed (`fine_grid` [Nf + 1]), the regular one when sample_stratified is off, else
        a fresh host-side draw shared by the rays.  In the union pass the tail's samples come from its own grid
        (corres.fine_grid), as in a separate render call: the grid is then per ray, [R, Nf + 1].  deterministic:
        ops.nerf_sample_pdf on the same grid instead of sample_depth_from_pdf + cat + sort."""
        opt, dev = self.net.opt, depth.device
        S, Nf = depth.shape[1], opt.nerf.sample_intvs_fine
        det = not opt.nerf.sample_stratified
        grid = fine_grid
        if corres is not None:
            grid = None
            if not det:
                gp = fine_grid if fine_grid is not None else torch.rand(Nf + 1)
                gc = corres.fine_grid if corres.fine_grid is not None else torch.rand(Nf + 1)
                grid = torch.cat([gp.to(dev).expand(Rp, Nf + 1), gc.to(dev).expand(depth.shape[0] - Rp, Nf + 1)])
        if not self.deterministic:
            fine_t = sample_depth_from_pdf(w[None], S, Nf, depth_range, det=det, grid=grid)
            return torch.cat([depth, fine_t[0, :, :, 0]], dim=1).sort(dim=1).values.contiguous()
        if grid is None:
            grid = torch.linspace(0, 1, Nf + 1, device=dev) if det else torch.rand(Nf + 1)
        out = torch.empty(depth.shape[0], S + Nf, dtype=torch.float32, device=dev)
        ops.nerf_sample_pdf(w, depth, grid.to(dev).float().contiguous(), Nf, depth_range, out)
        return out

    def optimizer_step(self, grad_scale=1.0):
        """torch.optim.Adam semantics (lib/utils.py:294-299); also re-zeroes the gradient blocks for the next step.  Like
        torch's optimiser, a network that received no gradient this iteration (the fine one before its start) is skipped and
        its step counter - hence its bias correction - does not advance."""
        self.step_count += 1
        for st in self.states:
            if not st.has_grad:
                continue
            st.steps += 1
            st.has_grad = False
            ops.adam_flat(st.net.flat, st.grad, st.m, st.v, st.seg_end, self.seg_lr, grad_scale, self.betas[0], self.betas[1],
                          self.eps, st.steps, True)

    def set_lr(self, lr):
        self.lr = lr
        self.seg_lr.fill_(lr)

    def step(self, center, ray, depth, image, **kw):
        loss, g_center, g_ray = self.forward_backward(center, ray, depth, image, **kw)
        self.optimizer_step()
        return loss, g_center, g_ray
