"""Pose initialisation of a joining view on the HIP path: the counterpart of the reference's `opencv_pnp_ransac`
(lib/recon_scene.py:276-310, called at :202-214 and :559-566), with PnP-RANSAC as HIP kernels (csrc/pp_pnp.hip) instead of
`cv2.solvePnPRansac`.

    from poseprobe_amd import pnp
    init = pnp.PnPInitialiser(engine, matches, Ks, render_kwargs)
    trainer = DualBranchTrainer(engine, opt, incremental_step=k, pose_initialiser=init)

Semantics (include/poseprobe_hip.h): the caller draws the samples, a hypothesis is a P3P solve on three rows
disambiguated by a fourth, the winner is the hypothesis with the most inliers (ties to the lowest index), its pose is refined by
Gauss-Newton on its inliers; fp64 inside, a pure and bit-reproducible function of its inputs.  `cv2`'s random draws, adaptive
iteration count, internal solver and Levenberg-Marquardt damping are not reproduced (none can be observed offline).  Nothing is
read back to the host: success or failure is decided on the device, and on failure the result is the fallback pose."""
import torch

from . import camera, ops, recon_utils

_KEY_BUDGET = 1 << 26          # random keys drawn at a time by draw_samples (256 MB of fp32)


def draw_samples(valid, n_hypotheses, generator=None):
    """[H,4] int32: four distinct rows with valid != 0 per hypothesis, uniformly, without a host read: every row gets a random
    key, invalid rows are pushed to the end, the four largest keys win (`multinomial` would raise on the host).  With fewer than
    four valid rows the hypotheses contain invalid rows, which the kernel marks invalid.  Works on CPU tensors too."""
    valid = torch.as_tensor(valid)
    P, H = int(valid.shape[0]), int(n_hypotheses)
    if P < 4:
        raise ValueError(f'draw_samples: at least 4 rows are needed (got {P})')
    if H < 1:
        raise ValueError('draw_samples: at least 1 hypothesis is needed')
    dead = (valid == 0)[None]
    out = []
    rows = max(1, _KEY_BUDGET // P)
    for h0 in range(0, H, rows):
        keys = torch.rand(min(rows, H - h0), P, generator=generator, device=valid.device)
        out.append(keys.masked_fill(dead, -1.0).topk(4, dim=1).indices)
    return torch.cat(out).to(torch.int32)


def intrinsics_rows(intr):
    """[V,3,3] camera matrices or [V,4] rows -> [V,4] rows (fx, fy, cx, cy)."""
    intr = torch.as_tensor(intr).float()
    if intr.shape[-2:] == (3, 3):
        intr = torch.stack([intr[..., 0, 0], intr[..., 1, 1], intr[..., 0, 2], intr[..., 1, 2]], -1)
    if intr.shape[-1] != 4:
        raise ValueError('intrinsics: [..., 3, 3] matrices or [..., 4] rows (fx, fy, cx, cy)')
    return intr


@torch.no_grad()
def solve_pnp_ransac(world, pix, intr, valid=None, n_hypotheses=256, reproj_error=8.0, refine_iters=10, min_inliers=6,
                     samples=None, generator=None, fallback=None):
    """world [P,3], pix [P,2] (pixel coordinates as cv2 takes them: inverse_y), intr [4] = (fx, fy, cx, cy), all on the device ->
    (w2c [3,4] fp32, inliers [P] uint8, info [2] int32 = (inlier count, winning hypothesis)), or (fallback, zeros, (0, -1)) when
    no hypothesis reaches min_inliers.  samples [H,4] int32 (default: draw_samples from `generator`); fallback defaults to the
    identity pose."""
    if not (isinstance(world, torch.Tensor) and world.is_cuda):
        raise RuntimeError('world must be a CUDA tensor')
    dev = world.device
    f = lambda t: t.detach().to(dev).float().contiguous()
    world, pix, intr = f(world), f(pix), f(intr).reshape(-1)
    P = world.shape[0]
    if valid is not None:
        valid = (valid.detach().to(dev) != 0).to(torch.uint8).contiguous()
    if samples is None:
        samples = draw_samples(torch.ones(P, dtype=torch.uint8, device=dev) if valid is None else valid, n_hypotheses, generator)
    samples = samples.detach().to(dev).to(torch.int32).contiguous()
    H = samples.shape[0]
    fallback = torch.eye(4, device=dev)[:3].contiguous() if fallback is None else f(fallback)
    with torch.cuda.device(dev):
        work = torch.empty(ops.pnp_workspace(P, H), dtype=torch.uint8, device=dev)
        w2c = torch.empty(3, 4, dtype=torch.float32, device=dev)
        inliers = torch.empty(P, dtype=torch.uint8, device=dev)
        info = torch.empty(2, dtype=torch.int32, device=dev)
        ops.pnp_ransac(world, pix, valid, intr, samples, reproj_error, refine_iters, min_inliers, fallback, work, w2c, inliers, info)
    return w2c, inliers, info


class PnPInitialiser:
    """`pose_initialiser` of trainer.DualBranchTrainer: (view, w2c_prev [3,4]) -> w2c [3,4] of the joining view, on the device.

    The reference's opencv_pnp_ransac restated: matches[view] = (pixels in the previous view [P,2], pixels in the new view [P,2],
    confidence [P]); the previous view's pixels are shot at the current surface (recon_utils.get_ray_dir(mode='no_center') with
    c2w = invert(w2c_prev), then model.query_sdf_point_wocuda(keep_dim=True)); valid = confidence * hit > 0; PnP-RANSAC on the
    surface points and the new view's pixels with fallback = w2c_prev - a view whose PnP fails starts where it starts without
    an initialiser.  model: a Voxurf, or a TrainEngine (read through voxurf_view(), so the surface is the current one).
    intr: [V,3,3] or [V,4].  DEVIATION: the reference hands Ks[0] to cv2 and Ks[view] to the rays for every view; here PnP uses
    the joining view's row and the rays the previous view's (where the pixels lie) - identical wherever intrinsics are shared.
    `last` = dict(info [2] int32, n_valid) as device tensors (logging; reading them synchronises)."""

    def __init__(self, model, matches, intr, render_kwargs, n_hypotheses=256, seed=0, reproj_error=8.0, refine_iters=10,
                 min_inliers=6):
        self.render_kwargs = dict(render_kwargs)
        self.flips = {k: self.render_kwargs.pop(k, v) for k, v in (('inverse_y', True), ('flip_x', False), ('flip_y', False))}
        if not self.flips['inverse_y']:
            raise NotImplementedError('PnPInitialiser: pixels are taken as cv2 takes them (inverse_y=True)')
        self.model, self.matches, self.intr = model, matches, intrinsics_rows(intr)
        self.n_hypotheses, self.seed = int(n_hypotheses), int(seed)
        self.reproj_error, self.refine_iters, self.min_inliers = float(reproj_error), int(refine_iters), int(min_inliers)
        self._view, self._gen = None, None
        self.last = None

    def _voxurf(self):
        if hasattr(self.model, 'voxurf_view'):
            self._view = self.model.voxurf_view(self._view)
            return self._view
        return self.model

    @torch.no_grad()
    def __call__(self, view, w2c_prev):
        model = self._voxurf()
        dev = model.sdf.grid.device
        prev = torch.as_tensor(w2c_prev, dtype=torch.float32).to(dev)[:3, :4].contiguous()
        pix_prev, pix_new, conf = (torch.as_tensor(t, dtype=torch.float32).to(dev) for t in self.matches[view][:3])
        P = int(pix_prev.shape[0])
        if P < 4:                                        # (a shape, not a device value: no synchronisation)
            self.last = dict(info=torch.tensor([0, -1], dtype=torch.int32, device=dev),
                             n_valid=torch.zeros((), dtype=torch.int64, device=dev))
            return prev.clone()
        if self._gen is None or self._gen.device != dev:
            self._gen = torch.Generator(device=dev).manual_seed(self.seed)
        rows = self.intr.to(dev)
        k_prev, k_new = rows[view - 1], rows[view].contiguous()
        K = torch.eye(3, device=dev)
        K[0, 0], K[1, 1], K[0, 2], K[1, 2] = k_prev[0], k_prev[1], k_prev[2], k_prev[3]
        o, d = recon_utils.get_ray_dir(pix_prev[None], K[None], c2w=camera.pose.invert(prev[None]), mode='no_center', **self.flips)
        world, hit, _ = model.query_sdf_point_wocuda(o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous(), global_step=None,
                                                     keep_dim=True, **self.render_kwargs, **self.flips)
        valid = ((conf * hit) > 0).to(torch.uint8)
        w2c, _, info = solve_pnp_ransac(world, pix_new, k_new, valid=valid, n_hypotheses=self.n_hypotheses,
                                        reproj_error=self.reproj_error, refine_iters=self.refine_iters,
                                        min_inliers=self.min_inliers, generator=self._gen, fallback=prev)
        self.last = dict(info=info, n_valid=valid.sum())
        return w2c
