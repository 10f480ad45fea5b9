"""The scores a run ends with, on the HIP path: SSIM / PSNR of rendered views and the rotation / translation error of the
optimised poses after aligning them to the ground-truth trajectory.

    from poseprobe_amd import evaluation
    s = evaluation.rgb_ssim(rgb, gt, max_val=1.)                       # lib/utils.py:792-838; device tensor, no host sync
    m = evaluation.image_metrics(rgbs, gts, masks)                     # psnr, psnr_fore, psnr_back, ssim: device tensors [V]
    r = evaluation.evaluate_viewpoints(model, w2c, cfg, HW, Ks, False, render_kwargs, gt_imgs, masks)
    error, aligned, sim3 = evaluation.evaluate_poses(w2c, w2c_GT)      # error.R in degrees, error.t x 100, per pose

SSIM is csrc/pp_ssim.hip (ops.ssim); the PSNRs and the pose functions are torch expressions on whatever device their inputs
are on.  The pose functions follow eval.py:539-550 and :699-821 of the reference (poses are [B,3,4] world-to-camera) but keep
the dtype they are given, where the reference's camera.pose casts to float32.  LPIPS is not provided: its network weights are
not part of this repository.

    poses = evaluation.refine_test_poses(net, opt, w2c_GT_test, sim3, images, Ks, depth_range)         # eval.py:1398-1408
    r = evaluation.evaluate_test_views(nerf, nerf_fine, opt, w2c, w2c_GT, w2c_GT_test, images, Ks, depth_range)

The held-out views of the scene branch follow the reference's protocol: their ground-truth poses are carried into the frame of
the optimised poses and refined photometrically against the frozen networks (pose_refine.py) before they are
rendered and scored.
"""
import numpy as np
import torch

from . import camera, nvs_fun, ops
from .losses import _AttrDict


# ------------------------------------------------------------------------------------------------------------- image scores
def _image_pair(x, y, names):
    """Two images as float32 contiguous CUDA tensors; shapes are checked before anything is uploaded."""
    shapes = [tuple(v.shape) if isinstance(v, torch.Tensor) else np.shape(v) for v in (x, y)]
    if len(shapes[0]) not in (3, 4):
        raise ValueError(f'{names[0]} must be [H,W,C] or [V,H,W,C], got {shapes[0]}')
    if shapes[0] != shapes[1]:
        raise ValueError(f'{names[0]} {shapes[0]} and {names[1]} {shapes[1]} differ in shape')
    dev = next((v.device for v in (x, y) if isinstance(v, torch.Tensor) and v.is_cuda), 'cuda')
    out = []
    for v in (x, y):
        t = v.detach() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
        out.append(t.to(dev).float().contiguous())
    return out


@torch.no_grad()
def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    """lib/utils.py:792-838 on [H,W,C] or [V,H,W,C] (C = 3 in the reference; 1..4 here), CUDA tensors or arrays (uploaded) -> a
    float32 device tensor, 0-dim or [V]: the mean of the SSIM map; with return_map the map [(V,) H - fs + 1, W - fs + 1, C]
    instead.  No host synchronisation."""
    shape = tuple(img0.shape) if isinstance(img0, torch.Tensor) else np.shape(img0)
    fs = int(filter_size)
    if len(shape) in (3, 4) and (shape[-3] < fs or shape[-2] < fs):
        raise ValueError(f'a {shape[-3]} x {shape[-2]} image is smaller than the filter ({fs})')
    a, b = _image_pair(img0, img1, ('img0', 'img1'))
    single = a.dim() == 3
    if single:
        a, b = a[None], b[None]
    V, H, W, C = a.shape
    if not 1 <= C <= 4:
        raise ValueError(f'{C} channels: 1 to 4 expected')
    if not 1 <= fs <= 33:
        raise ValueError(f'filter_size {fs} outside 1..33')
    if V < 1:
        raise ValueError('no view')
    with torch.cuda.device(a.device):
        work = torch.empty(ops.ssim_workspace(V, H, W, fs), dtype=torch.uint8, device=a.device)
        out = torch.empty(V, dtype=torch.float32, device=a.device)
        smap = torch.empty(V, H - fs + 1, W - fs + 1, C, dtype=torch.float32, device=a.device) if return_map else None
        ops.ssim(a, b, float(max_val), fs, float(filter_sigma), float(k1), float(k2), work, out, smap)
    if return_map:
        return smap[0] if single else smap
    return out[0] if single else out


@torch.no_grad()
def image_metrics(rgb, gt, mask=None, max_val=1.0):
    """rgb, gt [H,W,3] or [V,H,W,3], mask [(V,) H,W(,1)] or None -> dict of float32 device tensors (0-dim or [V]): psnr,
    psnr_fore, psnr_back in the reference's normalisation (lib/nvs_fun.py:118-123, nvs_fun.psnr_terms: the masked sums run over
    all channels and are divided by the masked PIXELS; fore / back are 0 without a mask) and ssim."""
    a, b = _image_pair(rgb, gt, ('rgb', 'gt'))
    single = a.dim() == 3
    a4, b4 = (a[None], b[None]) if single else (a, b)
    V = a4.shape[0]
    x, y = a4.double(), b4.double()
    psnr = -10. * torch.log10(((x - y) ** 2).reshape(V, -1).mean(1))
    fore = back = torch.zeros(V, dtype=torch.float64, device=a.device)
    if mask is not None:
        m = (mask.detach() if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask))))
        m = m.to(a.device).double()
        if m.dim() == (2 if single else 3):
            m = m[..., None]
        if single:
            m = m[None]
        if m.shape[:3] != a4.shape[:3]:
            raise ValueError(f'mask {tuple(mask.shape)} does not fit images {tuple(a.shape)}')
        back = -10. * torch.log10(((x * (1 - m) - y * (1 - m)) ** 2).reshape(V, -1).sum(1) / (1 - m).reshape(V, -1).sum(1))
        fore = -10. * torch.log10(((x * m - y * m) ** 2).reshape(V, -1).sum(1) / m.reshape(V, -1).sum(1))
    out = dict(psnr=psnr.float(), psnr_fore=fore.float(), psnr_back=back.float(), ssim=rgb_ssim(a4, b4, max_val))
    return {k: v[0] for k, v in out.items()} if single else out


@torch.no_grad()
def evaluate_viewpoints(model, render_poses, cfg, HW, Ks, ndc, render_kwargs, gt_imgs, masks=None, render_factor=0):
    """nvs_fun.render_viewpoints' views (same poses, intrinsics, flips, render_factor) rendered through nvs_fun.render_view,
    kept on the device and scored by image_metrics -> dict: psnr, psnr_fore, psnr_back, ssim (means over the views, floats),
    per_view (the same keys, lists) and rgbs (list of [H,W,3] device tensors).  One host copy, at the end."""
    dev = next(model.parameters()).device
    poses = torch.as_tensor(np.asarray(render_poses.cpu() if isinstance(render_poses, torch.Tensor) else render_poses),
                            dtype=torch.float32)
    if poses.shape[1] == 4:
        poses = poses[:, :3, :]
    if not (len(poses) == len(HW) == len(Ks) == len(gt_imgs)) or (masks is not None and len(masks) != len(poses)):
        raise ValueError('render_poses, HW, Ks, gt_imgs and masks must have one entry per view')
    c2ws = camera.pose.invert(poses).to(dev)
    HW, Ks = np.array(HW), np.array(Ks, dtype=np.float32)
    if render_factor != 0:
        HW = HW // render_factor
        Ks[:, :2, :3] //= render_factor
    flip_x = bool(getattr(getattr(cfg, 'data', None), 'flip_x', False))
    flip_y = bool(getattr(getattr(cfg, 'data', None), 'flip_y', False))
    keys = ('psnr', 'psnr_fore', 'psnr_back', 'ssim')
    rgbs, scores = [], []
    for i, c2w in enumerate(c2ws):
        H, W = int(HW[i][0]), int(HW[i][1])
        rgb = nvs_fun.render_view(model, H, W, torch.tensor(Ks[i], device=dev), c2w, ndc, render_kwargs, flip_x, flip_y,
                                  keys=('rgb_marched',))['rgb_marched']
        rgbs.append(rgb)
        m = image_metrics(rgb, gt_imgs[i], None if masks is None else masks[i])
        scores.append(torch.stack([m[k] for k in keys]))
    table = torch.stack(scores).cpu().numpy()                  # the host copy
    out = {k: float(table[:, j].mean()) for j, k in enumerate(keys)}
    out['per_view'] = {k: table[:, j].tolist() for j, k in enumerate(keys)}
    out['rgbs'] = rgbs
    return out


# --------------------------------------------------------------------------------------------------------------- pose error
def _poses(x, name):
    p = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    if p.dim() != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError(f'{name} must be [B,3,4], got {tuple(p.shape)}')
    p = p.detach()[:, :3]
    return p if p.is_floating_point() else p.float()


def _invert(pose):
    """[...,3,4] [R|t] -> [R^T | -R^T t], in the dtype of `pose`."""
    R_inv = pose[..., :3].transpose(-1, -2)
    return torch.cat([R_inv, -R_inv @ pose[..., 3:]], dim=-1)


def rotation_distance(R1, R2, eps=1e-7):
    """lib/camera.py:345-350: the angle of R1 R2^T in radians; the clamp keeps it at or above acos(1 - eps)."""
    R_diff = R1 @ R2.transpose(-2, -1)
    trace = R_diff[..., 0, 0] + R_diff[..., 1, 1] + R_diff[..., 2, 2]
    return ((trace - 1) / 2).clamp(-1 + eps, 1 - eps).acos()


@torch.no_grad()
def evaluate_camera_alignment(pose_aligned, pose_GT):
    """eval.py:539-550: [...,3,4] world-to-camera each -> R (degrees) and t (x 100) of the camera-to-world poses, per pose."""
    a, g = _invert(pose_aligned), _invert(pose_GT)
    R_error = rotation_distance(a[..., :3], g[..., :3]) * 180. / np.pi
    t_error = (a[..., 3] - g[..., 3]).norm(dim=-1) * 100
    return _AttrDict(R=R_error, t=t_error)


@torch.no_grad()
def prealign_w2c_small_camera_systems(pose_w2c, pose_GT_w2c):
    """eval.py:724-813: every ordered pair (a, b), a != b, among the first min(B, 10) poses gives a candidate - scale from the
    pair's baseline |c_GT[a] - c_GT[b]| / |c[a] - c[b]|, rigid transform from pose a - and the candidate with the lowest
    (mean t error) x (mean R error) wins, the first on ties.  All candidates are one batch; no host synchronisation.
    -> (aligned [B,3,4], sim3: R [1,3,3], t [1,3,1], s (0-dim tensor), type 'traj_align')."""
    pose, GT = _poses(pose_w2c, 'pose_w2c'), _poses(pose_GT_w2c, 'pose_GT_w2c')
    if pose.shape != GT.shape:
        raise ValueError(f'pose_w2c {tuple(pose.shape)} and pose_GT_w2c {tuple(GT.shape)} differ in shape')
    B = pose.shape[0]
    if B < 2:
        raise ValueError('prealign_w2c_small_camera_systems needs at least two poses')
    GT = GT.to(device=pose.device, dtype=pose.dtype)
    c2w, c2w_GT = _invert(pose), _invert(GT)
    n = min(B, 10)
    ia, ib = torch.meshgrid(torch.arange(n, device=pose.device), torch.arange(n, device=pose.device), indexing='ij')
    keep = ia != ib
    ia, ib = ia[keep], ib[keep]                                        # a-major, as the reference's double loop
    R, t, R_GT, t_GT = c2w[:, :, :3], c2w[:, :, 3], c2w_GT[:, :, :3], c2w_GT[:, :, 3]
    scale = (t_GT[ia] - t_GT[ib]).norm(dim=-1) / (t[ia] - t[ib]).norm(dim=-1)                          # [P]
    R_T = R_GT[ia] @ R[ia].transpose(-1, -2)                                                          # [P,3,3]
    t_T = t_GT[ia] - (R_T @ (t[ia] * scale[:, None])[..., None])[..., 0]                              # [P,3]
    R_al = R_T[:, None] @ R[None]                                                                     # [P,B,3,3]
    t_al = (R_T[:, None] @ (t[None] * scale[:, None, None])[..., None])[..., 0] + t_T[:, None]        # [P,B,3]
    aligned = _invert(torch.cat([R_al, t_al[..., None]], dim=-1))                                     # [P,B,3,4] world-to-camera
    error = evaluate_camera_alignment(aligned, GT[None])
    best = torch.argmin(error.t.mean(1) * error.R.mean(1)).reshape(1)
    sim3 = _AttrDict(R=R_T.index_select(0, best), t=t_T.index_select(0, best).reshape(1, 3, 1), s=scale.index_select(0, best)[0],
                     type='traj_align')
    return aligned.index_select(0, best)[0], sim3


def _umeyama(model, data):
    """external/ATE/align_trajectory.py align_umeyama: (s, R, t) with model = s R data + t, float64 numpy [N,3] each."""
    mu_M, mu_D = model.mean(0), data.mean(0)
    M, D = model - mu_M, data - mu_D
    n = model.shape[0]
    C = 1.0 / n * M.T @ D
    sigma2 = 1.0 / n * (D * D).sum()
    invalid = sigma2 < 1e-5
    if invalid:
        sigma2 = 1.
    U, d, Vt = np.linalg.svd(C)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1
    R = U @ S @ Vt
    s = 1. if invalid else 1.0 / (sigma2 + 1e-6) * np.trace(np.diag(d) @ S)
    return s, R, mu_M - s * R @ mu_D


@torch.no_grad()
def prealign_w2c_large_camera_systems(pose_w2c, pose_GT_w2c):
    """eval.py:699-720: the Sim(3) that maps the camera centres onto the ground truth's (Umeyama, as external/ATE does; float64
    on the host) applied to the camera-to-world poses; the identity transform if the SVD fails.
    -> (aligned [B,3,4], sim3: R [1,3,3], t [1,3,1], s (float), type 'traj_align')."""
    pose, GT = _poses(pose_w2c, 'pose_w2c'), _poses(pose_GT_w2c, 'pose_GT_w2c')
    if pose.shape != GT.shape:
        raise ValueError(f'pose_w2c {tuple(pose.shape)} and pose_GT_w2c {tuple(GT.shape)} differ in shape')
    c2w = _invert(pose.double().cpu()).numpy()
    c2w_GT = _invert(GT.double().cpu()).numpy()
    try:
        s, R, t = _umeyama(c2w_GT[:, :, 3], c2w[:, :, 3])
        if not (np.isfinite(s) and np.isfinite(R).all() and np.isfinite(t).all()):
            raise np.linalg.LinAlgError('non-finite alignment')
    except np.linalg.LinAlgError:
        s, R, t = 1., np.eye(3), np.zeros(3)
    al = np.concatenate([R[None] @ c2w[:, :, :3], s * (R[None] @ c2w[:, :, 3:]) + t[None, :, None]], axis=2)
    kw = dict(device=pose.device, dtype=pose.dtype)
    aligned = _invert(torch.from_numpy(al)).to(**kw)
    sim3 = _AttrDict(R=torch.from_numpy(R[None].copy()).to(**kw), t=torch.from_numpy(t.reshape(1, 3, 1).copy()).to(**kw), s=float(s),
                     type='traj_align')
    return aligned, sim3


@torch.no_grad()
def backtrack_from_aligning_the_trajectory(pose_GT_w2c, sim3):
    """eval.py:815-821: ground-truth poses carried into the frame of the optimised ones - the inverse of the alignment."""
    GT = _poses(pose_GT_w2c, 'pose_GT_w2c')
    c2w = _invert(GT)
    R, t = sim3.R.to(device=GT.device, dtype=GT.dtype), sim3.t.to(device=GT.device, dtype=GT.dtype)
    R_al = R.transpose(-2, -1) @ c2w[:, :, :3]
    t_al = R.transpose(-2, -1) / sim3.s @ (c2w[:, :, 3:4] - t)
    return _invert(torch.cat([R_al, t_al], dim=-1))


@torch.no_grad()
def evaluate_poses(pose_w2c, pose_GT_w2c):
    """eval.py:1353-1360: align (the trajectory alignment for more than 9 poses, the pair search otherwise) and measure
    -> (error: R [B] degrees, t [B] x 100; aligned [B,3,4]; sim3)."""
    pose, GT = _poses(pose_w2c, 'pose_w2c'), _poses(pose_GT_w2c, 'pose_GT_w2c')
    GT = GT.to(device=pose.device, dtype=pose.dtype)
    if pose.shape[0] > 9:
        aligned, sim3 = prealign_w2c_large_camera_systems(pose, GT)
    else:
        aligned, sim3 = prealign_w2c_small_camera_systems(pose, GT)
    return evaluate_camera_alignment(aligned, GT), aligned, sim3


# ------------------------------------------------------------------------------------------------- held-out views (scene branch)
def _per_view_K(Ks, T):
    K = Ks if isinstance(Ks, torch.Tensor) else torch.as_tensor(np.asarray(Ks))
    if K.dim() == 2:
        K = K[None].expand(T, 3, 3)
    if tuple(K.shape) != (T, 3, 3):
        raise ValueError(f'Ks must be [3,3] or [{T},3,3], got {tuple(K.shape)}')
    return K.float()


def refine_test_poses(net, opt, pose_GT_w2c_test, sim3, images, Ks, depth_range, return_losses=False, **refiner_kw):
    """eval.py:1398-1408: the ground-truth poses of the held-out views [T,3,4] carried into the frame of the optimised poses
    (backtrack_from_aligning_the_trajectory with `sim3` of evaluate_poses), then one photometric refinement per view against the
    frozen coarse network `net` (pose_refine.PoseRefiner.refine: 500 Adam steps by default), view after view as the reference runs
    them -> refined poses [T,3,4] on the networks' device (and, with return_losses, the losses [T, iters]).  images [T,H,W,3];
    Ks [3,3] or [T,3,3]; refiner_kw: `iters`, `generator` for refine(), the rest for PoseRefiner (rand_rays, lr, betas, eps)."""
    from . import pose_refine
    run_kw = {k: refiner_kw.pop(k) for k in ('iters', 'generator') if k in refiner_kw}
    base = backtrack_from_aligning_the_trajectory(_poses(pose_GT_w2c_test, 'pose_GT_w2c_test').to(net.flat.device), sim3)
    T = base.shape[0]
    if len(images) != T:
        raise ValueError(f'{len(images)} images for {T} poses')
    K = _per_view_K(Ks, T)
    H, W = images[0].shape[:2]
    refiner = pose_refine.PoseRefiner(net, opt, H, W, K[0], depth_range, **refiner_kw)
    poses, losses = [], []
    for i in range(T):
        refiner.set_intrinsics(K[i])
        image = images[i] if isinstance(images[i], torch.Tensor) else torch.as_tensor(np.asarray(images[i]))
        out = refiner.refine(base[i].float(), image, **run_kw)
        poses.append(out['pose_w2c'])
        losses.append(out['losses'])
    poses = torch.stack(poses)
    return (poses, torch.stack(losses)) if return_losses else poses


@torch.no_grad()
def evaluate_test_views(nerf, nerf_fine, opt, pose_w2c_train, pose_GT_w2c_train, pose_GT_w2c_test, images_test, Ks_test, depth_range,
                        refine=True, render='slices', chunk_rays=8192, **refiner_kw):
    """The scene branch's share of eval.py:1353-1416: evaluate_poses on the training poses; the held-out views' ground-truth
    poses backtracked into that frame and (refine=True) refined photometrically against the frozen coarse network; one full-view
    render per held-out view through bg_nerf.SceneRenderer.render_by_slices in mode 'val' - the fine network's colour where
    `nerf_fine` exists, else the coarse one; image_metrics.  One host copy, at the end.
    render='view': the renders go through SceneRenderer.render_view instead - forward-only kernels that keep no activation, the
    rays formed once per view, chunks of `chunk_rays` rays; the same images as 'slices' with opt.nerf.rand_rays = chunk_rays.
    -> dict: table [T,4] numpy (psnr, psnr_fore, psnr_back, ssim per view; fore / back are 0: no masks), poses_w2c [T,3,4] (device),
    error (R degrees, t x 100 of the aligned training poses), sim3, losses [T, iters] (device; None without refinement) and
    rgbs [T,H,W,3] (device).  Out of scope: the object branch's images of these views (evaluate_viewpoints renders them at any
    pose, poses_w2c included), LPIPS, multi-rank runs."""
    from . import bg_nerf
    if render not in ('slices', 'view'):
        raise ValueError(f"render = {render!r}: 'slices' or 'view'")
    error, _, sim3 = evaluate_poses(pose_w2c_train, pose_GT_w2c_train)
    dev = nerf.flat.device
    losses = None
    if refine:
        poses, losses = refine_test_poses(nerf, opt, pose_GT_w2c_test, sim3, images_test, Ks_test, depth_range, return_losses=True,
                                          **refiner_kw)
    else:
        poses = backtrack_from_aligning_the_trajectory(_poses(pose_GT_w2c_test, 'pose_GT_w2c_test').to(dev), sim3).float()
    T = poses.shape[0]
    K = _per_view_K(Ks_test, T).to(dev)
    ropt = opt
    if nerf_fine is None and opt.nerf.fine_sampling:              # a coarse-only render of a configuration that has a fine pass
        ropt = bg_nerf.Options(opt)
        ropt.nerf = bg_nerf.Options(opt.nerf)
        ropt.nerf.fine_sampling = False
    renderer = bg_nerf.SceneRenderer(ropt, nerf=nerf, nerf_fine=nerf_fine)
    keys = ('psnr', 'psnr_fore', 'psnr_back', 'ssim')
    rgbs, scores = [], []
    for i in range(T):
        H, W = images_test[i].shape[:2]
        if render == 'view':
            ret = renderer.render_view(ropt, poses[i:i + 1], H, W, K[i:i + 1], depth_range, mode='val', chunk_rays=chunk_rays)
        else:
            ret = renderer.render_by_slices(ropt, poses[i:i + 1], H, W, K[i:i + 1], depth_range, mode='val')
        rgb = (ret['rgb_fine'] if 'rgb_fine' in ret else ret['rgb']).view(H, W, 3)
        rgbs.append(rgb)
        m = image_metrics(rgb, images_test[i])
        scores.append(torch.stack([m[k] for k in keys]))
    table = torch.stack(scores).cpu().numpy()                  # the host copy
    return dict(table=table, poses_w2c=poses, error=error, sim3=sim3, losses=losses, rgbs=torch.stack(rgbs))
