"""Test-time pose refinement of a held-out view against FROZEN scene networks (eval.py:824-858, called from :1398-1416;
SPARF's original loop: lib/bg_nerf/source/models/renderer.py:1312-1337 and :911-935).

    refiner = PoseRefiner(net, opt, H, W, K, depth_range)
    out = refiner.refine(base_w2c, image)            # 500 Adam steps on a 6-vector; out['pose_w2c'] [3,4]

The reference does not score a test view at its ground-truth pose: it carries that pose into the frame of the optimised poses
(evaluation.backtrack_from_aligning_the_trajectory) and then minimises the photometric error of randomly drawn rays over a
left-composed SE(3) correction, `pose = compose([se3_to_SE3(se3), base])`, with Adam(lr = 5e-4) from se3 = 0.  One iteration
here is the same computation without autograd and without a parameter gradient:

    pp_pose_fwd (one view)  ->  randperm / stratified depths (torch's draws)  ->  pp_nerf_rays_select  ->  pp_nerf_fwd,
    pp_nerf_composite_fwd  ->  pp_nerf_mse_loss  ->  pp_nerf_composite_bwd, pp_nerf_bwd_input  ->  pp_nerf_c2w_fold, pp_pose_bwd
    ->  pp_adam_flat over the six numbers

The loss is taken on the COARSE network's colour, as the reference takes it on `rays_bg['rgb']`; a fine network is not run.
Nothing is read back and nothing synchronises inside the loop (the reference's loop reads no loss either).  The networks'
parameters, and the gradient / moment blocks of any SceneEngine that shares them, are not written: pp_nerf_bwd_input forms no
parameter gradient.  Out of scope: the fine network in the loss, batching several views into one pass, multi-rank runs, and
bit-reproducible draws (they are torch's).
"""
import numpy as np
import torch

from . import bg_nerf, ops


def check_intrinsics(K):
    """K as a float32 host tensor [3,3]; ValueError unless it is upper-triangular with K[2,2] = 1 (the closed-form inverse of
    pp_nerf_rays_select covers exactly that family, skew included)."""
    Kh = (K.detach().cpu() if isinstance(K, torch.Tensor) else torch.as_tensor(np.asarray(K))).float()
    if tuple(Kh.shape) != (3, 3):
        raise ValueError(f'K must be [3,3], got {tuple(Kh.shape)}')
    if float(Kh[1, 0]) != 0. or float(Kh[2, 0]) != 0. or float(Kh[2, 1]) != 0. or float(Kh[2, 2]) != 1. or \
            float(Kh[0, 0]) == 0. or float(Kh[1, 1]) == 0.:
        raise ValueError('K must be upper-triangular with K[2,2] = 1 and non-zero focal lengths: '
                         f'{Kh.tolist()}')
    return Kh.contiguous()


class PoseRefiner:
    def __init__(self, net, opt, H, W, K, depth_range, rand_rays=None, lr=5e-4, betas=(0.9, 0.999), eps=1e-8):
        """net: the coarse bg_nerf.NeRF (frozen here); K [3,3] upper-triangular with K[2,2] = 1, checked once (ValueError);
        rand_rays: rays per iteration, default opt.nerf.rand_rays, at most H * W.  Every per-iteration buffer is allocated once,
        at the first refine()."""
        self.K_host = check_intrinsics(K)
        self.net, self.opt, self.H, self.W = net, opt, int(H), int(W)
        if self.H < 1 or self.W < 1:
            raise ValueError(f'bad image size {H} x {W}')
        self.depth_range = (float(depth_range[0]), float(depth_range[1]))
        n = int(opt.nerf.rand_rays if rand_rays is None else rand_rays)
        if n < 1:
            raise ValueError(f'rand_rays = {n}')
        self.N, self.S = min(n, self.H * self.W), int(opt.nerf.sample_intvs)
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self._b = None

    def set_intrinsics(self, K):
        """Another view's K (same checks); the buffers stay."""
        self.K_host = check_intrinsics(K)
        if self._b is not None:
            self._b['K'].copy_(self.K_host)

    def _buffers(self):
        if self._b is None:
            dev, N = self.net.flat.device, self.N
            f = dict(dtype=torch.float32, device=dev)
            r3 = lambda: torch.empty(N, 3, **f)
            self._b = dict(
                K=self.K_host.to(dev), base=torch.empty(1, 3, 4, **f), se3=torch.zeros(1, 6, **f),
                m=torch.zeros(6, **f), v=torch.zeros(6, **f), se3_grad=torch.zeros(1, 6, **f),
                mask=torch.ones(1, dtype=torch.int32, device=dev), w2c=torch.empty(1, 3, 4, **f), c2w=torch.empty(1, 3, 4, **f),
                jac=torch.empty(1, 12, 6, **f), seg_end=torch.tensor([6], dtype=torch.int32, device=dev),
                seg_lr=torch.tensor([self.lr], **f), center=r3(), ray=r3(), dir_cam=r3(), target=r3(), g_rgb=r3(),
                g_c2w=torch.empty(1, 3, 4, **f))
        return self._b

    def _check(self, base_w2c, image, iters, replay):
        """Everything that can be refused, before anything is uploaded or allocated."""
        if int(iters) < 1:
            raise ValueError(f'iters = {iters}: at least one iteration')
        if tuple(base_w2c.shape) != (3, 4):
            raise ValueError(f'base_w2c must be [3,4], got {tuple(base_w2c.shape)}')
        if tuple(image.shape) != (self.H, self.W, 3):
            raise ValueError(f'image {tuple(image.shape)} does not fit the refiner ({self.H}, {self.W}, 3)')
        if replay is not None:
            idx, rnd = replay['ray_idx'], replay['depth_rand']
            if tuple(idx.shape) != (iters, self.N) or tuple(rnd.shape) != (iters, self.N, self.S):
                raise ValueError(f'replay: ray_idx [{iters},{self.N}] and depth_rand [{iters},{self.N},{self.S}] expected, got '
                                 f'{tuple(idx.shape)} and {tuple(rnd.shape)}')
            if idx.is_floating_point():
                raise ValueError('replay: ray_idx must be an integer tensor')
            if int(idx.min()) < 0 or int(idx.max()) >= self.H * self.W:
                raise ValueError(f'replay: ray_idx outside [0, {self.H * self.W})')

    def _backward(self, p, b, depth):
        """Compositing and network backward of the pass p w.r.t. the rays -> g_center, g_ray (tools/time_pose_refine.py swaps the
        full backward in here).  The loss gradient is all of the refiner's own g_rgb and no depth gradient: the pass may be the
        one a SceneEngine on the same network and shape uses, and nothing that user wrote is read."""
        return p.backward_input(b['ray'], depth, b['g_rgb'])

    @torch.no_grad()
    def refine(self, base_w2c, image, iters=500, generator=None, replay=None):
        """base_w2c [3,4] (the pose to correct: the backtracked ground-truth pose), image [H,W,3] -> dict of device tensors:
        pose_w2c [3,4] = compose([se3_to_SE3(se3), base_w2c]) of the returned se3 [6], losses [iters] (the MSE of every
        iteration's rays, before its update), se3_grad_first [6] (the first iteration's gradient).  se3 and the Adam state start
        from zero in every call.  generator: a torch.Generator of the networks' device for the draws; replay = dict(ray_idx
        [iters, N] integer, depth_rand [iters, N, S] in [0, 1)) replaces both draws (ray_idx outside [0, H * W): ValueError).
        The loss is the coarse network's; the returned pose is the one AFTER the last update (the reference keeps the pose of the
        last forward pass, one update earlier)."""
        iters = int(iters)
        self._check(base_w2c, image, iters, replay)
        net, opt, N, S, H, W = self.net, self.opt, self.N, self.S, self.H, self.W
        b = self._buffers()
        dev = net.flat.device
        p = net.scene_pass(N, S)
        image = image.detach().to(dev).float().contiguous()
        b['base'][0].copy_(base_w2c.detach().to(dev).float())
        for k in ('se3', 'm', 'v', 'se3_grad'):
            b[k].zero_()
        if replay is not None:
            idx_all = replay['ray_idx'].to(dev).to(torch.int32).contiguous()
            rand_all = replay['depth_rand'].to(dev).float()
        losses = torch.zeros(iters, dtype=torch.float32, device=dev)
        first = torch.zeros(6, dtype=torch.float32, device=dev)
        se3_flat, grad_flat = b['se3'].view(-1), b['se3_grad'].view(-1)
        for it in range(iters):
            ops.pose_fwd(b['se3'], b['base'], b['mask'], b['w2c'], b['c2w'], b['jac'])
            if replay is not None:
                ray_idx = idx_all[it]
                depth = bg_nerf.stratified_depths(opt, rand_all[it], self.depth_range).contiguous()
            else:
                ray_idx = torch.randperm(H * W, device=dev, generator=generator)[:N].to(torch.int32)
                depth = bg_nerf.sample_depth(opt, 1, N, S, self.depth_range, mode='train', device=dev,
                                             generator=generator).view(N, S)
            ops.nerf_rays_select(b['c2w'][0], b['K'], ray_idx, H, W, image, b['center'], b['ray'], b['dir_cam'], b['target'])
            p.forward(b['center'], b['ray'], depth)
            ops.nerf_mse_loss(p.rgb, b['target'], 1.0, losses[it:it + 1], b['g_rgb'])
            g_center, g_ray = self._backward(p, b, depth)
            ops.nerf_c2w_fold(g_ray[None], g_center[None], b['dir_cam'][None], b['g_c2w'])
            ops.pose_bwd(b['jac'], b['g_c2w'], b['se3_grad'])
            if it == 0:
                first.copy_(grad_flat)
            ops.adam_flat(se3_flat, grad_flat, b['m'], b['v'], b['seg_end'], b['seg_lr'], 1.0, self.betas[0], self.betas[1],
                          self.eps, it + 1, False)
        ops.pose_fwd(b['se3'], b['base'], b['mask'], b['w2c'], b['c2w'], b['jac'])
        return dict(pose_w2c=b['w2c'][0].clone(), se3=se3_flat.clone(), losses=losses, se3_grad_first=first)
