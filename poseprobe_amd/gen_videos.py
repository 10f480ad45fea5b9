"""Novel-view sequences of the scene branch: the camera paths of the reference's `generate_videos_synthesis`
(lib/bg_nerf/source/models/renderer.py:1213-1310, paths from lib/gen_videos.py:72-133 and lib/camera.py:371-381) and their frames
through the forward-only whole-view renderer (bg_nerf.SceneRenderer.render_view: pp_nerf_infer, no activation kept).

The two spiral generators work on the host in numpy float64, as the reference's do - a path is a few hundred 3 x 4 matrices
computed once per sequence -; the oscillation and every pose inversion are float32 torch (camera.pose).  Frames stay on the
device.  Out of scope: PNG / mp4 / gif files and colourised depth maps (matplotlib, ffmpeg).
"""
import numpy as np
import torch

from . import camera


def _unit(v):
    return v / np.linalg.norm(v)


def _look_along(z_dir, up, position):
    """Camera-to-world [3,4] of a camera at `position` whose z axis is z_dir (normalised here) and whose y axis is as close to
    `up` as orthogonality allows (lib/gen_videos.py:62-69)."""
    z = _unit(z_dir)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    return np.stack([x, y, z, position], axis=1)


def _mean_pose(poses):
    """The camera at the mean position with the mean z axis and mean up vector (lib/gen_videos.py:39-45)."""
    return _look_along(poses[:, :3, 2].mean(0), poses[:, :3, 1].mean(0), poses[:, :3, 3].mean(0))


def _focus_point(poses):
    """Least-squares nearest point to all optical axes (lib/gen_videos.py:48-54)."""
    d, o = poses[:, :3, 2:3], poses[:, :3, 3:4]
    m = np.eye(3) - d * np.transpose(d, [0, 2, 1])
    mtm = np.transpose(m, [0, 2, 1]) @ m
    return np.linalg.inv(mtm.mean(0)) @ (mtm @ o).mean(0)[:, 0]


def _as_numpy(poses_c2w):
    if isinstance(poses_c2w, torch.Tensor):
        return poses_c2w.detach().cpu().numpy(), True
    return np.asarray(poses_c2w), False


def _spiral(poses, radii, n_frames, n_rots, zrate, z_axis_of):
    """Positions radii * (cos, -sin, -sin(zrate theta), 1) in the mean camera's frame, theta over n_rots turns (end excluded);
    z_axis_of(position) -> (direction, subtract the position first?)."""
    radii = np.concatenate([radii, [1.]])
    mean, up = _mean_pose(poses), poses[:, :3, 1].mean(0)
    out = []
    for theta in np.linspace(0., 2. * np.pi * n_rots, n_frames, endpoint=False):
        position = mean @ (radii * [np.cos(theta), -np.sin(theta), -np.sin(theta * zrate), 1.])
        z, from_position = z_axis_of(mean, position)
        out.append(_look_along(z - position if from_position else z, up, position))
    return np.stack(out, axis=0)


def generate_spiral_path(poses_c2w, bounds, n_frames=240, n_rots=2, zrate=.5):
    """Forward-facing spiral (lib/gen_videos.py:72-105): poses_c2w [V,3,4] (OpenCV convention), bounds = depth bounds; radii =
    90th percentile of |position| per axis, every camera looks from the point at the focus depth (a disparity-weighted mean of
    0.9 x the nearest and 5 x the farthest bound) in front of the mean camera.  -> [n_frames,3,4], a float64 tensor for a
    tensor input, else numpy."""
    poses, is_torch = _as_numpy(poses_c2w)
    bounds = np.asarray(bounds)
    close, far, dt = bounds.min() * .9, bounds.max() * 5., .75
    focal = 1 / ((1 - dt) / close + dt / far)
    radii = np.percentile(np.abs(poses[:, :3, 3]), 90, 0)
    path = _spiral(poses, radii, n_frames, n_rots, zrate, lambda mean, position: (position - mean @ [0, 0, -focal, 1.], False))
    return torch.from_numpy(path)[:, :3] if is_torch else path


def generate_spiral_path_dtu(poses_c2w, n_frames=240, n_rots=2, zrate=.5, perc=60):
    """The DTU spiral (lib/gen_videos.py:108-133): radii = the perc-th percentile of |position|, every camera looks at the
    point nearest to all input optical axes."""
    poses, is_torch = _as_numpy(poses_c2w)
    radii = np.percentile(np.abs(poses[:, :3, 3]), perc, 0)
    focus = _focus_point(poses)
    path = _spiral(poses, radii, n_frames, n_rots, zrate, lambda mean, position: (focus, True))
    return torch.from_numpy(path)[:, :3] if is_torch else path


def centre_most(poses_w2c):
    """Index of the pose whose translation column is nearest to the mean one (renderer.py:1260)."""
    return (poses_w2c - poses_w2c.mean(dim=0, keepdim=True))[..., 3].norm(dim=-1).argmin()


def novel_view_poses(poses_w2c, dataset, n_frames=60, depth_range=None):
    """World-to-camera poses of the novel-view sequence (renderer.py:1236-1275) from the views' poses_w2c [V,3,4]:
    'llff' in dataset: the forward-facing spiral (n_frames; needs depth_range); 'dtu': the DTU spiral with one turn followed by
    the oscillation around the centre-most camera (2 x n_frames); anything else: the oscillation alone (n_frames).  float32,
    on poses_w2c's device."""
    dev = poses_w2c.device
    poses_w2c = poses_w2c.float()
    if 'llff' in dataset:
        if depth_range is None:
            raise ValueError("novel_view_poses: the 'llff' spiral needs depth_range")
        c2w = generate_spiral_path(camera.pose.invert(poses_w2c), bounds=np.array(depth_range, dtype=np.float64), n_frames=n_frames)
        return camera.pose.invert(c2w.to(dev))
    oscillation = camera.get_novel_view_poses(None, poses_w2c[centre_most(poses_w2c)], N=n_frames, scale=1)
    if 'dtu' in dataset:
        c2w = generate_spiral_path_dtu(camera.pose.invert(poses_w2c), n_rots=1, n_frames=n_frames)
        return torch.cat((camera.pose.invert(c2w.to(dev)), oscillation), dim=0)
    return oscillation


@torch.no_grad()
def render_novel_views(renderer, opt, poses_w2c, intr, H, W, depth_range, dataset='dtu', n_frames=60, chunk_rays=8192):
    """The frames of the novel-view sequence: novel_view_poses(poses_w2c, dataset, n_frames), each rendered in mode 'val' by
    renderer.render_view with the first view's intrinsics (intr [3,3] or [V,3,3]), the fine network's outputs where the fine
    pass is active.  -> dict(poses_w2c [F,3,4], rgb [F,H,W,3], depth [F,H,W]) on the device; no host read."""
    dev = renderer.device
    poses = novel_view_poses(poses_w2c.to(dev), dataset, n_frames=n_frames, depth_range=depth_range)
    K = torch.as_tensor(intr, dtype=torch.float32).to(dev).reshape(-1, 3, 3)[:1]
    F = poses.shape[0]
    rgb = torch.empty(F, H, W, 3, dtype=torch.float32, device=dev)
    depth = torch.empty(F, H, W, dtype=torch.float32, device=dev)
    for f in range(F):
        ret = renderer.render_view(opt, poses[f:f + 1], H, W, K, depth_range, mode='val', chunk_rays=chunk_rays)
        sfx = '_fine' if 'rgb_fine' in ret else ''
        rgb[f].copy_(ret['rgb' + sfx].view(H, W, 3))
        depth[f].copy_(ret['depth' + sfx].view(H, W))
    return dict(poses_w2c=poses, rgb=rgb, depth=depth)
