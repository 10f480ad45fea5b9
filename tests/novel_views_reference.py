"""Inputs of the novel-view pose-path tests, regenerated from a seed (nothing of them is stored): tools/make_novel_views_golden.py
feeds them to the reference's own path functions and records the outputs in tests/golden/novel_view_poses.npz;
tests/test_scene_view_host.py feeds them to poseprobe_amd.gen_videos / camera and compares."""
import numpy as np

N_SPIRAL = 8           # frames of the recorded spirals (two turns: n_rots = 2, the functions' default)
N_PATH = 6             # n_frames of the recorded oscillations and composed paths


def _look_at_w2c(centre, target, up):
    z = target - centre
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z], axis=0)                 # world -> camera rotation (rows = camera axes)
    return np.concatenate([R, (-R @ centre)[:, None]], axis=1)


def cases():
    """-> [dict(name, poses_w2c [V,3,4] float64, bounds [2] float64, scale)]: cameras on a cap of a sphere around a point near the
    origin, looking at it with a little jitter - three views (the DTU protocol), nine, and a wide forward-facing rig."""
    out = []
    for name, seed, V, radius, cap, scale in (('three', 11, 3, 2.4, 0.35, 1), ('nine', 12, 9, 3.1, 0.6, 1), ('rig', 13, 5, 1.2, 0.15, 0.5)):
        rng = np.random.RandomState(seed)
        target = rng.randn(3) * 0.1
        poses = []
        for _ in range(V):
            d = np.array([0.0, 0.0, -1.0]) + rng.randn(3) * cap
            centre = target + radius * (1 + 0.1 * rng.randn()) * d / np.linalg.norm(d)
            up = np.array([0.0, -1.0, 0.0]) + rng.randn(3) * 0.05
            poses.append(_look_at_w2c(centre, target + rng.randn(3) * 0.05, up))
        out.append(dict(name=name, poses_w2c=np.stack(poses), bounds=np.array([0.5 * radius, 1.6 * radius]), scale=scale))
    return out


def invert(poses):
    """[...,3,4] float64 world-to-camera <-> camera-to-world."""
    Rt = np.swapaxes(poses[..., :3], -1, -2)
    return np.concatenate([Rt, -Rt @ poses[..., 3:]], axis=-1)
