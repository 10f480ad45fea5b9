"""Minimal counterpart of the reference's joint training loop (lib/recon_scene.py:534-791) around the two HIP engines: the
schedules that decide WHAT a step does, the batch samplers and the scene branch's snapshot file.  Not a re-implementation of
the trainer (view selection, PnP re-initialisation, matching, logging and evaluation stay with the reference): it exists to
drive `joint.DualBranchEngine` the way `scene_rep_reconstruction` drives the two models, and to read / write the files that
loop reads / writes.

Schedules (all pure functions of the step, unit-tested on the CPU):
  * scene learning rate   ExponentialLR from `optim.lr` to `optim.lr_end` over `max_iter` (lib/utils.py:300-313,
                          default_config.py:176-180),
  * coarse-to-fine window `progress = iteration_nerf / max_iter` written into both NeRFs (renderer.py:399-402),
  * fine network          from `ratio_start_fine_sampling_at_x * max_iter` on (renderer.py:580-584),
  * pose refinement       while `step < ratio_end_joint_nerf_pose_refinement * max_iter` (sparf.py:33, recon_scene.py:770),
  * scene objective       `opt.loss_type` (loss_factory.py:25-42): the photometric term, plus SPARF's correspondence term
                          weighted 10^loss_weight.corres / gamma from `start_iter.corres` on (corres_loss.py:78-90, :151).
"""
import os
import random

import numpy as np
import torch

from . import bg_nerf, ops
from .joint import DualBranchEngine


def scene_lr(step, lr=1e-3, lr_end=1e-4, max_iter=60000):
    """Learning rate the scheduler holds AFTER `step` optimiser steps."""
    gamma = (lr_end / lr) ** (1.0 / max_iter)
    return lr * gamma ** step


def fine_phase(step, max_iter, ratio_start_fine=0.3, fine_sampling=True):
    return bool(fine_sampling) and not (ratio_start_fine is not None and step < max_iter * ratio_start_fine)


def pose_phase(step, max_iter, ratio_end_pose=0.3):
    return step < max_iter * ratio_end_pose


def c2f_progress(iteration_nerf, max_iter):
    return iteration_nerf / max_iter


def active_views(global_step, n_views, incremental_step, incremental=True, start=2):
    """Number of views in play at `global_step`: the incremental schedule of lib/recon_scene.py:552-576 starts from the first
    two views and takes in one more whenever the step count reaches a multiple of `cfg.camera.incremental_step` (the
    check runs before the step's batch is drawn, never at step 0) until all views are in."""
    if not incremental or incremental_step <= 0:
        return n_views
    return int(min(n_views, start + max(global_step, 0) // incremental_step))


def object_phase(global_step, n_iters_object, start_object=0):
    """The object branch is optimised while start_object <= step <= cfg_train.N_iters (lib/recon_scene.py:584)."""
    return start_object <= global_step <= n_iters_object


SCENE_TERMS = ('photometric', 'corres', 'depth_cons')


def loss_terms(loss_type):
    """`opt.loss_type` -> the set of scene-branch terms (loss_factory.py:25-42 builds one module per '_and_'-joined name).
    None / absent = 'photometric', the objective before loss_type was read.  'depth_cons' is accepted and adds NOTHING:
    the reference's DepthConsistencyLoss.compute_loss (depth_cons_loss.py:128-230) computes its loss into a local variable
    and returns the empty loss_dict it created on entry, so no depth_cons key ever reaches the weighted sum
    (base_losses.py:37-55) - its renders cost time there and change no parameter update."""
    if loss_type is None or loss_type == '':
        return frozenset(['photometric'])
    names = str(loss_type).split('_and_')
    unknown = [n for n in names if n not in SCENE_TERMS]
    if unknown:
        raise NotImplementedError(f'scene loss term(s) {unknown} of loss_type {loss_type!r} are not implemented '
                                  f'(supported: {" / ".join(SCENE_TERMS)})')
    if 'photometric' not in names:
        raise NotImplementedError(f'loss_type {loss_type!r}: the scene branch always trains the photometric term')
    return frozenset(names)


def loss_weight(opt, key):
    """Weight of term `key` (base_losses.py:111-130): 10^w under the 'exp' parametrization, w otherwise; None = term off."""
    lw = getattr(opt, 'loss_weight', None)
    if lw is None:
        return 1.0 if key == 'photometric' else None
    if lw.get('equalize_losses', False):
        raise NotImplementedError('loss_weight.equalize_losses is not implemented')
    w = lw.get('render' if key == 'photometric' else key)
    if w is None:
        return None
    return 10 ** float(w) if lw.get('parametrization', 'exp') == 'exp' else float(w)


def corres_gamma(iteration, opt, max_iter):
    """Divisor of the correspondence weight (corres_loss.py:78-90): 2^((iteration - start) // corres_weight_reduct_at_x_iter)
    from start = ratio_start_decrease_corres_weight * max_iter (or iter_start_decrease_corres_weight) on, 1 before."""
    if not getattr(opt, 'gradually_decrease_corres_weight', False):
        return 1.0
    ratio = getattr(opt, 'ratio_start_decrease_corres_weight', None)
    start = ratio * max_iter if ratio is not None else getattr(opt, 'iter_start_decrease_corres_weight', 0)
    if iteration < start:
        return 1.0
    return float(2 ** ((iteration - start) // getattr(opt, 'corres_weight_reduct_at_x_iter', 10000)))


def corres_started(iteration, opt):
    """The term is skipped while iteration < start_iter.corres (corres_loss.py:151)."""
    st = getattr(opt, 'start_iter', None)
    return iteration >= (st.get('corres', 0) if st is not None else 0)


def pair_partner(i):
    """Partner of view i in the scene matches: i - 1, and 1 for view 0 (setup_matcher_results with num_camera = 1,
    recon_scene.py:225-245)."""
    return 1 if i == 0 else i - 1


def pair_table(scene_matches):
    """scene_matches[i] = (pix_self [P,2], pix_other [P,2], conf [P]) or with an explicit partner as a 4th entry (None = the
    default rule) -> [(i, j, pix_self, pix_other, conf)], keeping the rows with conf > 0 (corres_loss.py:160-162: the mask is
    applied here, once, so that no step has a data-dependent shape)."""
    table = []
    for i, entry in enumerate(scene_matches):
        if entry is None:
            table.append(None)
            continue
        ps, po, conf = entry[:3]
        j = pair_partner(i) if len(entry) < 4 or entry[3] is None else int(entry[3])
        conf = torch.as_tensor(conf).reshape(-1)
        keep = conf > 0
        table.append((i, j, torch.as_tensor(ps)[keep], torch.as_tensor(po)[keep], conf[keep]))
    return table


def corres_sample_size(n_matches, rand_rays):
    """Matched rows rendered per step: all of them up to rand_rays // 2, a random subset of that many beyond
    (corres_loss.py:171-176)."""
    return min(int(n_matches), int(rand_rays) // 2)


def reproj_sample_size(n_matches, reproj_rows):
    """Matches of the drawn pair that take part in a step of the engine-native reprojection pass: all of them up to
    reproj_rows // 2 (each match is two rows, one per direction), a random subset of that many beyond."""
    return min(int(n_matches), int(reproj_rows) // 2)


def surface_projection_active(global_step, max_iter, ratio_end_pose, n_iters_object, start_object=0):
    """The surface-projection feature term joins the object loss while the object branch is optimised AND poses are
    (`weight_surface_projection > 0 and IsOptimizePose` inside `if optimize_object_nerf`, lib/recon_scene.py:594, :610)."""
    return object_phase(global_step, n_iters_object, start_object) and pose_phase(global_step, max_iter, ratio_end_pose)


def surface_projection_pair(rng, pairs, n_active):
    """One (i, j) of `pairs` whose views are both among the first n_active, drawn from the numpy RandomState `rng`
    (lib/recon_scene.py:611-612 draws an index into the pair table); None - and no draw - while no pair is live."""
    live = [(int(i), int(j)) for i, j in pairs if i < n_active and j < n_active]
    if not live:
        return None
    return live[rng.randint(len(live))]


def surface_projection_sample_size(n_rays, H, W):
    """Rays of a step of the term: min(256, H W) in the reference (lib/recon_scene.py:372)."""
    return min(int(n_rays), int(H) * int(W))


def _term_options(name, given, obj_engine, deterministic, **defaults):
    """The option dict `name`= of DualBranchTrainer (an auxiliary term of the object loss on the engine's own launches) with the
    defaults filled in and 'rng', the RandomState(seed) its view pair is drawn from; refused beside deterministic=True."""
    if deterministic or getattr(obj_engine, 'deterministic', False):
        raise ValueError(f'{name}= is out of the scope of deterministic=True (its render backward keeps float atomics)')
    r = dict(defaults, seed=0, n_iters_object=obj_engine.cfg.N_iters, start_object=0)
    r.update(given)
    r['rng'] = np.random.RandomState(r['seed'])
    return r


class DualBranchTrainer:
    def __init__(self, obj_engine, opt, max_iter=60000, lr=1e-3, lr_end=1e-4, ratio_start_fine=0.3, ratio_end_pose=0.3,
                 depth_range=(0.5, 3.0), seed=0, incremental_step=0, pose_initialiser=None, scene_matches=None,
                 deterministic=False, reprojection=None, surface_projection=None):
        """incremental_step > 0: the incremental view schedule (`active_views`); a view that joins gets its initial pose from
        `pose_initialiser(view, w2c_of_previous_view [3,4]) -> w2c [3,4]` - the reference's PnP hand-off (cv2.solvePnPRansac on
        matcher output, lib/recon_scene.py:202-214, :276-310) plugs in here: `pnp.PnPInitialiser` is its counterpart on the HIP
        path (PnP-RANSAC kernels, the previous pose as the fallback); the default is its `use_identical` variant (the
        previous view's current pose).
        scene_matches: per view i, (pix_self [P,2], pix_other [P,2], conf [P][, partner]) - the reference's coord1_scene[i],
        coord0_scene[i], mconf_scene[i] (recon_scene.py:247-257), paired with view pair_partner(i) unless a partner is given;
        read when opt.loss_type contains 'corres'.
        deterministic: passed to DualBranchEngine (needs a deterministic, single-GPU obj_engine): the joint step's own sums run
        in fixed orders.  Out of its scope: `reprojection`, `surface_projection` and multi-rank runs.
        reprojection: dict(pairs, nl, weight_projection, weight_near_surface, pixel_thre=200, seed=0) - the reprojection +
        near-surface terms of the object loss (lib/recon_scene.py:621-637; configs/dtu_e2e/scan1.py:60-61: 1e-3 / 1e-1) inside
        the engine's own launches (TrainEngine.reprojection_grads): complete gradients (pose, and from the third active view on
        the warp network and sdf_alpha / sdf_beta), no autograd, no host synchronisation.  pairs: (i, j, coord_i [P,2],
        coord_j [P,2], conf [P]), matcher output; one pair among the active views is drawn per step from RandomState(seed), both
        directions of its matches are the step's rows; mode 'render' iff more than two views are active (:584); active in the
        object phase only (`object_phase(global_step, n_iters_object, start_object)`; optional keys n_iters_object - default: the
        engine's cfg.N_iters - and start_object = 0).  obj_engine must have been built with reproj_rows > 0, the row
        capacity: matches beyond reproj_rows // 2 are subsampled on the device, a fresh subset every step - a DEVIATION from
        the reference, which uses every match.  The capacity costs one second render workspace: about 18 KB per sample, i.e.
        18 KB * n_samples per row (160^3 voxels, 186 samples: 3.4 MB per row, 1024 rows = 512 matches: 3.5 GB).
        surface_projection: dict(features, pairs, weight, nl, n_rays=256, seed=0) - the surface-based feature term of the object
        loss (lib/recon_scene.py:371-439, :610-619; configs/dtu_e2e: weight_surface_projection = 1e-3) inside the engine's own
        launches (TrainEngine.surface_projection_grads).  features: the per-view feature maps, a list of [V,C,h,w] (the reference's
        VGG features - an input here, as the matcher's output is); pairs: the (i, j) view pairs.  Per step one pair among the active
        views is drawn from RandomState(seed) and min(n_rays, H W) pixels of view 0 - the reference always shoots from the first
        training view - on the device; active only while `surface_projection_active` holds (optional keys n_iters_object -
        default: the engine's cfg.N_iters - and start_object = 0).  obj_engine must have been built with featproj_rows >=
        min(n_rays, H W); the capacity costs 18.4 KB * n_samples per row (TrainEngine).  last_featproj records the pair and the row
        count of the step, or None."""
        self.opt, self.max_iter = opt, max_iter
        self.terms = loss_terms(getattr(opt, 'loss_type', None))
        self.photo_weight = loss_weight(opt, 'photometric') if 'loss_type' in opt else 1.0
        if self.photo_weight != 1.0:
            raise NotImplementedError('loss_weight.render other than 10^0 is not implemented')
        self.corres_weight = None
        if 'corres' in self.terms:
            self.corres_weight = loss_weight(opt, 'corres')
            if scene_matches is None:
                raise ValueError(f'loss_type {opt.loss_type!r} needs scene_matches')
        self.pairs = None if scene_matches is None or self.corres_weight is None else [
            None if p is None else (p[0], p[1], *(t.float().to(obj_engine.dev) for t in p[2:]))
            for p in pair_table(scene_matches)]
        self.pair_rng = random.Random(seed)
        self.last_scene_terms = None
        self.incremental_step, self.pose_initialiser = incremental_step, pose_initialiser
        self.n_active = None
        self.reprojection = None
        if reprojection is not None:
            if getattr(obj_engine, 'reproj_rows', 0) < 2:
                raise ValueError('reprojection= needs an object engine built with reproj_rows >= 2')
            r = _term_options('reprojection', reprojection, obj_engine, deterministic, pixel_thre=200)
            fl = lambda t: torch.as_tensor(t, dtype=torch.float32).to(obj_engine.dev)
            r['pairs'] = [(int(i), int(j), fl(ci), fl(cj), fl(cf)) for i, j, ci, cj, cf in r['pairs']]
            self.reprojection = r
        self.last_reproj = None
        self.surface_projection = None
        if surface_projection is not None:
            r = _term_options('surface_projection', surface_projection, obj_engine, deterministic, n_rays=256)
            r['n'] = surface_projection_sample_size(r['n_rays'], obj_engine.H, obj_engine.W)
            if getattr(obj_engine, 'featproj_rows', 0) < r['n']:
                raise ValueError(f"surface_projection= needs an object engine built with featproj_rows >= {r['n']}")
            obj_engine.set_feature_maps(r.pop('features'))
            r['pairs'] = [(int(i), int(j)) for i, j in r['pairs']]
            r['gen'] = torch.Generator(device=obj_engine.dev).manual_seed(r['seed'])
            self.surface_projection = r
        self.last_featproj = None
        self.lr, self.lr_end = lr, lr_end
        self.ratio_start_fine, self.ratio_end_pose = ratio_start_fine, ratio_end_pose
        dev = obj_engine.dev
        self.nerf = bg_nerf.NeRF(opt, device=dev)
        self.nerf_fine = bg_nerf.NeRF(opt, is_fine_network=True, device=dev) if opt.nerf.fine_sampling else None
        self.joint = DualBranchEngine(obj_engine, self.nerf, lr_scene=lr, depth_range=depth_range, scene_net_fine=self.nerf_fine,
                                      deterministic=deterministic)
        self.iteration = 0            # == the reference's Graph.iteration_nerf
        self.gen = torch.Generator(device=dev).manual_seed(seed)
        self.dev = dev

    # ---- batches (recon_scene.py:598-606 for the object branch, sampling_strategies.py:132-170 for the scene branch) ------
    def sample_batch(self, n_active=None):
        """Object-branch rays are a prefix of a permutation of the ACTIVE views' pixels (views 0 .. n_active - 1 are
        contiguous in the flattened [V, H, W] order); the scene branch draws rand_rays // n_active pixels per active view."""
        e = self.joint.obj
        k = e.V if n_active is None else n_active
        n_total = k * e.H * e.W
        ray_idx = torch.randperm(n_total, device=self.dev, generator=self.gen)[:e.N].to(torch.int32)
        jitter = torch.rand(e.N, device=self.dev, generator=self.gen)
        n_pix = self.opt.nerf.rand_rays // k
        flat = torch.randperm(e.H * e.W, device=self.dev, generator=self.gen)[:n_pix]
        py, px = flat // e.W, flat % e.W
        image = e.images[:k, py, px]                                   # [k, n_pix, 3] ground-truth colours at those pixels
        pixels = torch.stack([px.float() + 0.5, py.float() + 0.5], dim=-1)
        return ray_idx, jitter, pixels, image

    def _admit_views(self, global_step):
        """Incremental schedule: views joining at this step start from a handed-over pose with zero refinement."""
        e = self.joint.obj
        k = active_views(global_step, e.V, self.incremental_step, self.incremental_step > 0)
        if self.n_active is None:
            self.n_active = k if self.incremental_step <= 0 else min(k, 2)
        while self.n_active < k:
            v = self.n_active
            ops.pose_fwd(e.se3, e.w2c_init, e.refine_mask, e.w2c, e.c2w, e.jac)          # current pose of the previous view
            prev = e.w2c[v - 1].detach().clone()
            init = prev if self.pose_initialiser is None else torch.as_tensor(self.pose_initialiser(v, prev.cpu()),
                                                                              dtype=torch.float32).to(e.dev)
            with torch.no_grad():
                e.w2c_init[v].copy_(init[:3, :4])
                e.se3[v].zero_(); e.se3_m[v].zero_(); e.se3_v[v].zero_()
            self.n_active += 1
        return self.n_active

    def _corres_batch(self, global_step, k):
        """The correspondence rows of this step, or None: one view drawn uniformly among the k active ones with its partner
        (recon_scene.py:642-644; `iteration` of the loss is the joint loop's global_step, :643), its matches subsampled on the
        device to rand_rays // 2 (corres_loss.py:171-176), weight 10^loss_weight.corres / gamma."""
        if self.pairs is None or not corres_started(global_step, self.opt):
            return None
        v = self.pair_rng.randrange(k)
        entry = self.pairs[v] if v < len(self.pairs) else None
        if entry is None:
            return None
        i, j, ps, po, conf = entry
        if j >= k or ps.shape[0] == 0:                      # an explicit partner that is not in play yet / no match left
            return None
        n = corres_sample_size(ps.shape[0], self.opt.nerf.rand_rays)
        if n < ps.shape[0]:
            sel = torch.randperm(ps.shape[0], device=self.dev, generator=self.gen)[:n]
            ps, po, conf = ps[sel], po[sel], conf[sel]
        return dict(i=i, j=j, pix_self=ps, pix_other=po, conf=conf, opt=self.opt,
                    weight=self.corres_weight / corres_gamma(global_step, self.opt, self.max_iter))

    def _reproj_batch(self, global_step, k):
        """The reprojection rows of this step, or None: one live pair drawn on the host, both directions of its matches as rows -
        own view j first, get_project_error's order -, subsampled on the device to reproj_rows // 2 matches.  Shapes depend on host
        values only."""
        r = self.reprojection
        if r is None:
            return None
        if not object_phase(global_step, r['n_iters_object'], r['start_object']):
            return None
        live = [p for p in r['pairs'] if p[0] < k and p[1] < k]
        if not live:
            return None
        i, j, ci, cj, conf = live[r['rng'].randint(len(live))]           # the draw is over ALL live pairs, empty ones included
        if ci.shape[0] == 0:                                               # a drawn pair without matches: no term this step
            return None
        n = reproj_sample_size(ci.shape[0], self.joint.obj.reproj_rows)
        if n < ci.shape[0]:
            sel = torch.randperm(ci.shape[0], device=self.dev, generator=self.gen)[:n]
            ci, cj, conf = ci[sel], cj[sel], conf[sel]
        own = torch.cat([torch.full((n,), j, dtype=torch.int32, device=self.dev), torch.full((n,), i, dtype=torch.int32, device=self.dev)])
        other = torch.cat([torch.full((n,), i, dtype=torch.int32, device=self.dev), torch.full((n,), j, dtype=torch.int32, device=self.dev)])
        rows = dict(own=own, other=other, pix=torch.cat([cj, ci]).contiguous(), match=torch.cat([ci, cj]).contiguous(),
                    conf=torch.cat([conf, conf]).contiguous())
        self.last_reproj = dict(pair=(i, j), mode='render' if k > 2 else 'crossing', n_rows=2 * n)
        return dict(rows=rows, mode=self.last_reproj['mode'], weight_projection=r['weight_projection'],
                    weight_near_surface=r['weight_near_surface'], nl=r['nl'], pixel_thre=r['pixel_thre'])

    def _featproj_batch(self, global_step, k):
        """The surface-projection rows of this step, or None: one live pair drawn on the host, the pixels of view 0 on the device
        (through their centres).  Shapes depend on host values only."""
        r = self.surface_projection
        if r is None or not surface_projection_active(global_step, self.max_iter, self.ratio_end_pose, r['n_iters_object'],
                                                      r['start_object']):
            return None
        pair = surface_projection_pair(r['rng'], r['pairs'], k)
        if pair is None:
            return None
        e, n = self.joint.obj, r['n']
        flat = torch.randperm(e.H * e.W, device=self.dev, generator=r['gen'])[:n]
        pix = torch.stack([(flat % e.W).float() + 0.5, (flat // e.W).float() + 0.5], dim=-1).contiguous()
        rows = dict(src=torch.zeros(n, dtype=torch.int32, device=self.dev), pix=pix, own=pair[0], other=pair[1])
        self.last_featproj = dict(pair=pair, n_rows=n)
        return dict(rows=rows, weight=r['weight'], nl=r['nl'])

    def train_step(self, global_step):
        """One iteration of the joint loop; returns (object-branch summary, scene loss)."""
        self.iteration += 1
        k = self._admit_views(global_step)
        fine = fine_phase(global_step, self.max_iter, self.ratio_start_fine, self.nerf_fine is not None)
        ray_idx, jitter, pixels, image = self.sample_batch(k)
        corres = self._corres_batch(global_step, k)
        self.last_reproj = None
        reproj = self._reproj_batch(global_step, k)
        extra = {} if reproj is None else {'reproj': reproj}
        self.last_featproj = None
        featproj = self._featproj_batch(global_step, k)
        if featproj is not None:
            extra['featproj'] = featproj
        out = self.joint.train_step(ray_idx, jitter, global_step, pixels, image, fine=fine,
                                    optimize_pose=pose_phase(global_step, self.max_iter, self.ratio_end_pose), n_views=k,
                                    corres=corres, **extra)
        self.last_scene_terms = self.joint.last_scene_terms
        self.joint.scene.set_lr(scene_lr(self.iteration, self.lr, self.lr_end, self.max_iter))
        p = c2f_progress(self.iteration, self.max_iter)                # takes effect from the next iteration (renderer.py:399)
        self.nerf.progress.data.fill_(p)
        if self.nerf_fine is not None:
            self.nerf_fine.progress.data.fill_(p)
        return out

    def _active_poses(self):
        """-> k, w2c [k,3,4]: the active views' current poses, the engine's w2c refreshed from the pose parameters as the head of
        the next step refreshes it."""
        e = self.joint.obj
        k = e.V if self.n_active is None else self.n_active
        ops.pose_fwd(e.se3, e.w2c_init, e.refine_mask, e.w2c, e.c2w, e.jac)
        return k, e.w2c[:k].detach()

    def pose_error(self, pose_GT_w2c):
        """Rotation (degrees) / translation (x 100) error of the active views' current poses against pose_GT_w2c [>= k,3,4] after
        aligning them to it (evaluation.evaluate_poses; the number lib/recon_scene.py:664-668 logs): -> (error, aligned, sim3).
        Not part of train_step; it refreshes the engine's w2c from the pose parameters, as the head of the next step does."""
        from . import evaluation
        k, w2c = self._active_poses()
        return evaluation.evaluate_poses(w2c, torch.as_tensor(pose_GT_w2c)[:k, :3])

    def evaluate_test_views(self, pose_GT_w2c_train, pose_GT_w2c_test, images_test, Ks_test, **kw):
        """Held-out views by the reference's protocol (eval.py:1353-1416; evaluation.evaluate_test_views with this trainer's
        networks, the active views' current poses and its depth range): alignment of the training poses, test-time pose
        refinement against the frozen scene networks (refine=False skips it), full-view renders, PSNR / SSIM.  The networks and
        the optimiser state are left as they are.  render='view' (optionally chunk_rays=) renders through the forward-only
        SceneRenderer.render_view."""
        from . import evaluation
        k, w2c = self._active_poses()
        return evaluation.evaluate_test_views(self.nerf, self.nerf_fine, self.opt, w2c, torch.as_tensor(pose_GT_w2c_train)[:k, :3],
                                              pose_GT_w2c_test, images_test, Ks_test, self.joint.depth_range, **kw)

    def novel_views(self, intr, H, W, dataset='dtu', n_frames=60, chunk_rays=8192):
        """The novel-view sequence of the reference's generate_videos_synthesis (renderer.py:1213-1310) around the active views'
        current poses, rendered by this trainer's networks at its depth range (gen_videos.render_novel_views):
        -> dict(poses_w2c [F,3,4], rgb [F,H,W,3], depth [F,H,W]) on the device.  Networks and optimiser state are not written."""
        from . import gen_videos
        _, w2c = self._active_poses()
        renderer = bg_nerf.SceneRenderer(self.opt, nerf=self.nerf, nerf_fine=self.nerf_fine)
        return gen_videos.render_novel_views(renderer, self.opt, w2c, intr, H, W, self.joint.depth_range,
                                             dataset=dataset, n_frames=n_frames, chunk_rays=chunk_rays)

    def export_mesh(self, cfg, **kw):
        """The mesh export the reference's training loop ends its object phase with (lib/recon_scene.py:748-751):
        dtu_eval.validate_deform_mesh on the object engine's CURRENT parameters, read through its drop-in view
        (TrainEngine.voxurf_view: built once, re-pointed at the live buffers on every call) -> the driver's return value.
        global_step (the BARF weights of the colour pass with extract_color=True) defaults to the object engine's step count;
        the other keyword arguments are validate_deform_mesh's - among them keep= ('largest', a triangle count or a fraction of
        the largest component), which drops the mesh's stray connected components on the device before it is shaded, written and
        scored (mesh.keep_components).  The engine and the optimiser state are left as they are."""
        from . import dtu_eval
        e = self.joint.obj
        self._mesh_view = e.voxurf_view(getattr(self, '_mesh_view', None))
        kw.setdefault('global_step', e.n_step)
        return dtu_eval.validate_deform_mesh(self._mesh_view, cfg, **kw)

    # ---- `model_last.pth.tar` (renderer.py:1028-1051 save_snapshot, recon_scene.py:827-838 load) ----------------------------
    def _adam_state_dict(self):
        """torch.optim.Adam.state_dict() layout over [nerf.parameters(), nerf_fine.parameters()] (lib/utils.py:294-299)."""
        state, groups, idx = {}, [], 0
        for st in self.joint.scene.states:
            ids = []
            views_m, views_v = st.net._views(st.m), st.net._views(st.v)
            for m, v in zip(views_m, views_v):
                if st.steps > 0:
                    state[idx] = {'step': torch.tensor(float(st.steps)), 'exp_avg': m.detach().clone().cpu(),
                                  'exp_avg_sq': v.detach().clone().cpu()}
                ids.append(idx)
                idx += 1
            ids.append(idx)                                            # `progress`: a Parameter without gradient, no state
            idx += 1
            groups.append({'lr': float(self.joint.scene.lr), 'betas': (0.9, 0.999), 'eps': 1e-8, 'weight_decay': 0,
                           'amsgrad': False, 'params': ids})
        return {'state': state, 'param_groups': groups}

    def state_dict(self):
        sd = {'nerf.' + k: v.detach().clone().cpu() for k, v in self.nerf.state_dict().items()}
        if self.nerf_fine is not None:
            sd.update({'nerf_fine.' + k: v.detach().clone().cpu() for k, v in self.nerf_fine.state_dict().items()})
        return sd

    def save_snapshot(self, directory, filename='model_last.pth.tar'):
        os.makedirs(directory, exist_ok=True)
        e = self.joint.obj
        torch.save({'current_pose': e.w2c.detach().clone().cpu(), 'epoch': 0, 'iteration': self.iteration,
                    'iteration_nerf': self.iteration, 'state_dict': self.state_dict(), 'best_val': None,
                    'epoch_of_best_val': None, 'optimizer': self._adam_state_dict(),
                    'scheduler': {'last_epoch': self.iteration, 'gamma': (self.lr_end / self.lr) ** (1.0 / self.max_iter),
                                  '_last_lr': [float(self.joint.scene.lr)] * len(self.joint.scene.states)}},
                   os.path.join(directory, filename))

    def load_snapshot(self, path):
        """Accepts a file written by save_snapshot or by the reference's Graph.save_snapshot (tensors only are read)."""
        ck = torch.load(path, map_location='cpu', weights_only=True)
        sd = ck['state_dict']
        nets = [('nerf.', self.nerf)] + ([('nerf_fine.', self.nerf_fine)] if self.nerf_fine is not None else [])
        for prefix, net in nets:
            net.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
        self.iteration = int(ck['iteration_nerf'])
        opt_state, groups = ck['optimizer']['state'], ck['optimizer']['param_groups']
        for st, grp in zip(self.joint.scene.states, groups):
            ids = grp['params'][:-1]
            st.m.zero_(), st.v.zero_()
            st.steps = 0
            for i, m, v in zip(ids, st.net._views(st.m), st.net._views(st.v)):
                if i in opt_state:
                    m.copy_(opt_state[i]['exp_avg'])
                    v.copy_(opt_state[i]['exp_avg_sq'])
                    st.steps = int(opt_state[i]['step'])
        self.joint.scene.set_lr(scene_lr(self.iteration, self.lr, self.lr_end, self.max_iter))
        return ck.get('current_pose')
