"""Dual-branch optimisation step: object branch (voxel SDF renderer, engine.TrainEngine) and scene branch (NeRF MLP,
bg_nerf.SceneEngine) driven by ONE set of camera poses, `loss = 0.1 * L_obj + L_bg` (lib/recon_scene.py:645-649), one
optimiser step for each parameter group (:765-771).

The pose is shared the way the reference shares it (`model_bg.data_dict.poses_w2c = current_pose[train_idx]`, :639): the
object engine's pose kernel produces c2w and its Jacobian d c2w / d se3 once per step; the scene branch's rays are the
(per-ray, tiny) camera algebra of lib/bg_nerf/source/utils/camera.py:384-416 on that c2w, and the scene branch's ray
gradients are folded back through the same Jacobian, so se3 receives the sum of both branches' gradients before its Adam
step.
"""
import torch

from . import bg_nerf, ops


class DualBranchEngine:
    def __init__(self, obj_engine, scene_net, lr_scene=1e-3, depth_range=(0.5, 3.0), scene_net_fine=None, deterministic=False):
        """deterministic=True: bit-reproducible joint step.  Needs a deterministic single-GPU object engine
        (TrainEngine(deterministic=True), no `dist`; ValueError otherwise), builds a deterministic bg_nerf.SceneEngine and folds
        the scene branch's ray gradients into the pose gradient with ops.nerf_c2w_fold (fixed order) instead of torch's einsum /
        sum.  GUARANTEE (the conditions of TrainEngine's): identical state, ray_idx, jitter, global_step, pixels, image, replayed
        depth_rand / fine_grid / corres_rand / corres_fine_grid and the same corres rows give, after every train_step, bit-identical
        k0, k0_m, k0_v, flat.data, flat.m, flat.v, se3, se3_m, se3_v of the object engine and flat, m, v of the coarse and the
        fine scene network - coarse phase, hierarchical phase, and both with the correspondence term.  Not covered: the
        engine-native reprojection and surface-projection passes (forward_backward(reproj=... / featproj=...): refused with
        ValueError), multi-rank runs, and bg_nerf.SceneRenderer's autograd route.  Off (default): nothing changes."""
        self.deterministic = bool(deterministic)
        if self.deterministic:
            if not getattr(obj_engine, 'deterministic', False):
                raise ValueError('DualBranchEngine: deterministic=True with an object engine built without deterministic=True '
                                 '(its gradients keep float atomics, and both branches feed one pose update)')
            if getattr(obj_engine, 'dist', None) is not None:
                raise ValueError('DualBranchEngine: deterministic=True with a multi-rank object engine (dist) is not covered: '
                                 'the exchange keeps its own reductions')
        self.obj = obj_engine
        self.scene = bg_nerf.SceneEngine(scene_net, lr=lr_scene, net_fine=scene_net_fine, deterministic=self.deterministic)
        self.depth_range = depth_range
        e = obj_engine
        self._se3_tmp = torch.zeros_like(e.se3_grad)
        self.last_scene_loss = None
        self.last_scene_terms = None
        self._K = None

    def scene_rays(self, pixels, n_views=None):
        """pixels [N, 2] (x, y; the same for every view, as the reference's sampler draws them) -> center, ray [V, N, 3] and
        the camera-frame directions [V, N, 3] for the pose chain (the first n_views views when the trainer's incremental
        schedule has not admitted all of them yet)."""
        e = self.obj
        k = e.V if n_views is None else n_views
        fx, fy, cx, cy = (e.intr[:k, i][:, None] for i in range(4))
        x, y = pixels[None, :, 0], pixels[None, :, 1]
        dir_cam = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like((x - cx) / fx)], dim=-1)
        c2w = e.c2w[:k]
        ray = dir_cam @ c2w[:, :, :3].transpose(-1, -2)
        center = c2w[:, None, :, 3].expand_as(ray)
        return center, ray, dir_cam

    def intrinsics(self):
        """[V,3,3] intrinsic matrices of the object engine's views, rebuilt only when its intrinsics change."""
        e = self.obj
        key = (e.intr.data_ptr(), e.intr._version)
        if self._K is None or self._K[0] != key:
            K = torch.zeros(e.V, 3, 3, device=e.intr.device)
            K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = e.intr[:, 0], e.intr[:, 1], e.intr[:, 2], e.intr[:, 3], 1.
            self._K = (key, K)
        return self._K[1]

    def pair_rays(self, i, j, pix_self, pix_other):
        """Rays of the matched pixels of views (i, j) (bg_nerf.get_center_and_ray_at_pixels: K^-1 [x, y, 1], no half-pixel
        offset) on the current c2w -> center, ray, dir_cam [2, M, 3] (self rows, then other rows)."""
        e = self.obj
        pix = torch.stack([pix_self, pix_other])
        fx, fy, cx, cy = (torch.stack([e.intr[i], e.intr[j]])[:, k][:, None] for k in range(4))
        x, y = pix[..., 0], pix[..., 1]
        dir_cam = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)], dim=-1)
        c2w = torch.stack([e.c2w[i], e.c2w[j]])
        ray = dir_cam @ c2w[:, :, :3].transpose(-1, -2)
        return c2w[:, None, :, 3].expand_as(ray), ray, dir_cam

    def forward_backward(self, ray_idx, jitter, global_step, pixels, image, depth_rand=None, fine=False, fine_grid=None,
                         n_views=None, corres=None, corres_rand=None, corres_fine_grid=None, reproj=None, featproj=None):
        """ray_idx / jitter: the object branch's batch (engine.TrainEngine.train_step); pixels [N, 2] + image [V, N, 3]: the
        scene branch's batch; depth_rand [V, N, S, 1] / fine_grid [Nf + 1] optionally replay the samplers' draws.  On return every gradient
        buffer (object engine's k0 / MLPs / se3 - the pose gradient of BOTH branches - and the scene engine's block) is
        filled; the object engine's gradients must be zero on entry (its optimiser kernels leave them so).
        corres: dict(i, j, pix_self [M,2], pix_other [M,2], conf [M], weight, opt=None, photo_weight=1.0) adds SPARF's
        correspondence term of the view pair (i, j) (corres_loss.py:140-222, weight = 10^-2 / gamma in the reference's DTU
        setting): its rows render in the same scene launches as the photometric rays, L_bg = photometric + weight * corres
        (last_scene_terms holds both parts); corres_rand [2, M, S, 1] / corres_fine_grid [Nf + 1] replay its draws.
        reproj: dict(rows, mode, weight_projection, weight_near_surface, nl, pixel_thre, jitter=None) adds the object loss's
        reprojection + near-surface terms (lib/recon_scene.py:621-637) through engine.TrainEngine.reprojection_grads (the object
        engine needs reproj_rows > 0): loss_scale * (weight_near_surface * near + weight_projection * err) joins the object
        branch's gradients - the pose, and in mode 'render' the warp network and sdf_alpha / sdf_beta; the object engine's
        last_reproj_terms holds the scalars as device tensors.
        featproj: dict(rows, weight, nl, jitter=None, jitter_ref=None) adds the object loss's surface-projection feature term
        (lib/recon_scene.py:610-619) through engine.TrainEngine.surface_projection_grads (the object engine needs featproj_rows > 0
        and feature maps): loss_scale * weight * L joins the object branch's gradients - the pose, the warp network and sdf_alpha /
        sdf_beta; the object engine's last_featproj_terms holds the scalars as device tensors.  Runs beside `reproj`, with the same
        refusals."""
        e, sc = self.obj, self.scene
        if corres is not None and e.dist is not None:
            raise NotImplementedError('DualBranchEngine: the correspondence term is not sharded across ranks')
        for key, name, term in (('reproj', 'reprojection', reproj), ('featproj', 'surface-projection', featproj)):
            if term is None:
                continue
            if self.deterministic or getattr(e, 'deterministic', False):
                raise ValueError(f'DualBranchEngine: {key} is out of the scope of deterministic=True (its render backward keeps float '
                                 'atomics)')
            if e.dist is not None:
                raise NotImplementedError(f'DualBranchEngine: the {name} term is not sharded across ranks')
        out = e.render_and_grads(ray_idx, jitter, global_step)            # also refreshes e.c2w / e.jac for this step
        if reproj is not None:
            e.reprojection_grads(reproj['rows'], reproj['mode'], global_step, jitter=reproj.get('jitter'),
                                 weight_projection=reproj['weight_projection'], weight_near_surface=reproj['weight_near_surface'],
                                 nl=reproj['nl'], pixel_thre=reproj.get('pixel_thre'))
        if featproj is not None:
            e.surface_projection_grads(featproj['rows'], global_step, featproj['weight'], featproj['nl'], jitter=featproj.get('jitter'),
                                       jitter_ref=featproj.get('jitter_ref'))
        opt = sc.net.opt
        V, N, S = (e.V if n_views is None else n_views), pixels.shape[0], opt.nerf.sample_intvs
        center, ray, dir_cam = self.scene_rays(pixels, V)

        def depths(rand, n_views, n_rays):                  # [n_views, n_rays, S, 1]: a fresh draw, or a replayed one
            if rand is None:
                return bg_nerf.sample_depth(opt, n_views, n_rays, S, self.depth_range, mode='train', device=pixels.device)
            return bg_nerf.stratified_depths(opt, rand, self.depth_range)

        center, ray, depth = center.reshape(V * N, 3), ray.reshape(V * N, 3), depths(depth_rand, V, N).reshape(V * N, S)
        rows = None
        if corres is not None:
            i, j = int(corres['i']), int(corres['j'])
            if not (0 <= i < V and 0 <= j < V and i != j):
                raise ValueError(f'DualBranchEngine: correspondence pair ({i}, {j}) is not a pair of the {V} views in play')
            M = corres['pix_self'].shape[0]
            c_center, c_ray, c_dir = self.pair_rays(i, j, corres['pix_self'], corres['pix_other'])
            K = self.intrinsics()
            rows = bg_nerf.CorresRows(corres['pix_self'], corres['pix_other'], corres['conf'], K[i], K[j], e.w2c[i], e.w2c[j],
                                      corres['weight'], opt=corres.get('opt', opt), fine_grid=corres_fine_grid,
                                      photo_weight=corres.get('photo_weight', 1.0))
            center, ray = torch.cat([center, c_center.reshape(2 * M, 3)]), torch.cat([ray, c_ray.reshape(2 * M, 3)])
            depth = torch.cat([depth, depths(corres_rand, 2, M).reshape(2 * M, S)])
        loss_bg, g_center, g_ray = sc.forward_backward(center.contiguous(), ray.contiguous(), depth.contiguous(),
                                                       image.reshape(V * N, 3), fine=fine, depth_range=self.depth_range,
                                                       fine_grid=fine_grid, corres=rows)
        # fold the ray gradients into d L_bg / d c2w and through the object engine's pose Jacobian
        g_ray_p, g_center_p = g_ray[:V * N].view(V, N, 3), g_center[:V * N].view(V, N, 3)
        if self.deterministic:                          # fixed summation order; views that are not in play receive zeros
            g_c2w = torch.empty(e.V, 3, 4, dtype=torch.float32, device=g_ray.device)
            ops.nerf_c2w_fold(g_ray_p, g_center_p, dir_cam.contiguous(), g_c2w)
        else:
            g_c2w = torch.cat([torch.einsum('vni,vnj->vij', g_ray_p, dir_cam), g_center_p.sum(1)[..., None]], dim=-1)
            if V < e.V:                                     # views that are not in play yet receive no scene gradient
                g_c2w = torch.cat([g_c2w, torch.zeros(e.V - V, 3, 4, device=g_c2w.device)], dim=0)
            g_c2w = g_c2w.contiguous()
        if corres is not None:
            # the matched rows' ray gradients and the loss's direct gradient on both w2c, accumulated into views i and j
            ops.nerf_pair_pose_bwd(g_center[V * N:], g_ray[V * N:], c_dir.reshape(2 * M, 3), e.w2c, sc.last_g_w2c, i, j, g_c2w)
            self.last_scene_terms = sc.last_terms
        else:
            self.last_scene_terms = None
        ops.pose_bwd(e.jac, g_c2w, self._se3_tmp)
        e.se3_grad += self._se3_tmp
        self.last_scene_loss = loss_bg
        return out, loss_bg

    def train_step(self, ray_idx, jitter, global_step, pixels, image, depth_rand=None, optimize_pose=True, fine=False,
                   fine_grid=None, n_views=None, corres=None, reproj=None, featproj=None):
        """fine=True: the scene branch also runs its fine network (after ratio_start_fine_sampling_at_x of the schedule).
        corres, reproj, featproj: see forward_backward."""
        extra = {k: v for k, v in (('corres', corres), ('reproj', reproj), ('featproj', featproj)) if v is not None}
        out = self.forward_backward(ray_idx, jitter, global_step, pixels, image, depth_rand, fine, fine_grid, n_views, **extra)
        e = self.obj
        e.grad_scale = 1.0
        if e.dist is not None:
            # ray-sharded data parallelism: the object engine's exchange already carries se3_grad, which holds
            # the pose gradient of BOTH branches; the scene networks add one 2 MB all-reduce each (averaged by grad_scale)
            e.dist.reduce_gradients(e)
            for st in self.scene.states:
                if st.has_grad:
                    e.dist.all_reduce_tensor(st.grad)
        e.optimizer_step(optimize_pose, grad_scale=e.grad_scale)
        self.scene.optimizer_step(grad_scale=e.grad_scale)
        if e.dist is not None:
            e.dist.gather_parameters(e)
        return out
