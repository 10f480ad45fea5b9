"""Test-time pose refinement restated in float64 torch on the CPU (a helper, not a test): one iteration and the loop of
poseprobe_amd/pose_refine.py with plain autograd on oracle.scene_nerf.render - se3_to_SE3, compose, invert, rays, F.mse_loss,
torch.optim.Adam - plus the small seeded problem the GPU tests and this helper share, so that the convergence condition of the
trajectory test can be checked without a GPU:

    python tests/pose_refine_reference.py          # prints the loss of the first / last ten iterations of the seeded problem

Conventions (lib/camera.py:51-142 of the reference, eval.py:815-858): poses are [3,4] world-to-camera, x_cam = R x + t;
compose([a, b]) applies a first (R = R_b R_a, t = R_b t_a + t_b); the refined pose is compose([se3_to_SE3(se3), base]).
"""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import scene_nerf as SN  # noqa: E402

f64 = torch.float64


# ------------------------------------------------------------------------------------------------------------ pose algebra
def _series(x2, first):
    """sum_i (-1)^i x^(2i) / (2i + first)!  - sin(x)/x (first = 1), (1 - cos x)/x^2 (2), (x - sin x)/x^3 (3) as power series in
    x^2: smooth at 0, where the loop starts."""
    out, term = 0., 1. / math.factorial(first)
    for i in range(12):
        out = out + term
        term = term * (-x2) / ((2 * i + first + 1) * (2 * i + first + 2))
    return out


def skew(w):
    O = torch.zeros((), dtype=w.dtype)
    return torch.stack([torch.stack([O, -w[2], w[1]]), torch.stack([w[2], O, -w[0]]), torch.stack([-w[1], w[0], O])])


def se3_to_SE3(wu):
    """[6] = (rotation vector, u) -> [3,4] = [exp(w^) | V u]."""
    w, u = wu[:3], wu[3:]
    wx, x2 = skew(w), (w * w).sum()
    I = torch.eye(3, dtype=wu.dtype)
    A, B, C = _series(x2, 1), _series(x2, 2), _series(x2, 3)
    R = I + A * wx + B * wx @ wx
    V = I + B * wx + C * wx @ wx
    return torch.cat([R, (V @ u)[:, None]], dim=1)


def compose_pair(a, b):
    return torch.cat([b[:, :3] @ a[:, :3], b[:, :3] @ a[:, 3:] + b[:, 3:]], dim=1)


def invert(p):
    Rt = p[:, :3].T
    return torch.cat([Rt, -Rt @ p[:, 3:]], dim=1)


def refined_pose(se3, base_w2c):
    return compose_pair(se3_to_SE3(se3), base_w2c)


def backtrack(pose_GT_w2c, R, t, s):
    """eval.py:815-821 for one pose: the ground-truth pose carried into the optimised poses' frame by the inverse of the
    Sim(3) (R [3,3], t [3], s) that aligned the optimised camera-to-world poses to the ground truth."""
    c2w = invert(pose_GT_w2c)
    return invert(torch.cat([R.T @ c2w[:, :3], (R.T / s) @ (c2w[:, 3:] - t.reshape(3, 1))], dim=1))


def held_out_pose(se3, pose_GT_w2c, R, t, s):
    """eval.py:824-835: compose([se3_to_SE3(se3), backtrack(GT)])."""
    return refined_pose(se3, backtrack(pose_GT_w2c, R, t, s))


# -------------------------------------------------------------------------------------------------------------------- rays
def rays(pose_w2c, K, ray_idx, W):
    """Pixel centres (idx % W + 0.5, idx // W + 0.5) -> center, ray [N,3], dir_cam [N,3] (utils/camera.py:347-416)."""
    x = (ray_idx % W).to(pose_w2c.dtype) + 0.5
    y = torch.div(ray_idx, W, rounding_mode='floor').to(pose_w2c.dtype) + 0.5
    dir_cam = torch.stack([x, y, torch.ones_like(x)], dim=-1) @ torch.linalg.inv(K).T
    c2w = invert(pose_w2c)
    return c2w[:, 3].expand(len(ray_idx), 3), dir_cam @ c2w[:, :3].T, dir_cam


def depths(rand, depth_range):
    S = rand.shape[-1]
    return (rand + torch.arange(S, dtype=rand.dtype)) / S * (depth_range[1] - depth_range[0]) + depth_range[0]


def iteration_loss(P, se3, base_w2c, K, image, ray_idx, rand, depth_range, progress, barf_c2f, white_bg=False):
    """The loss of one iteration (eval.py:847-853) as a differentiable function of se3 [6]."""
    W = image.shape[1]
    center, ray, _ = rays(refined_pose(se3, base_w2c), K, ray_idx, W)
    out = SN.render(P, center, ray, depths(rand, depth_range), progress, barf_c2f, white_bg=white_bg)
    return F.mse_loss(out['rgb'], image.reshape(-1, 3)[ray_idx])


def loop(P, base_w2c, K, image, ray_idx, rand, depth_range, progress, barf_c2f, lr=5e-4, white_bg=False):
    """eval.py:838-858 with replayed draws ray_idx [iters,N], rand [iters,N,S] -> (se3 after every iteration [iters,6], losses
    [iters], first gradient [6])."""
    se3 = torch.zeros(6, dtype=base_w2c.dtype, requires_grad=True)
    optim = torch.optim.Adam([se3], lr=lr)
    hist, losses, first = [], [], None
    for it in range(ray_idx.shape[0]):
        optim.zero_grad()
        loss = iteration_loss(P, se3, base_w2c, K, image, ray_idx[it], rand[it], depth_range, progress, barf_c2f, white_bg)
        loss.backward()
        if first is None:
            first = se3.grad.detach().clone()
        optim.step()
        hist.append(se3.detach().clone())
        losses.append(loss.detach())
    return torch.stack(hist), torch.stack(losses), first


# ------------------------------------------------------------------------------------------------- the shared seeded problem
H, W, S, PROGRESS, BARF_C2F, DEPTH_RANGE = 12, 16, 24, 0.565, (0.4, 0.7), (0.5, 3.0)
SEED = 3
PERTURBATION = (0.03, -0.02, 0.025, 0.04, -0.03, 0.02)          # se3 of the base pose's error: ~2.5 degrees, ~5 % of the depth


def seeded_params(seed=SEED):
    """A state dict of bg_nerf.NeRF's shapes drawn on the CPU (Xavier-uniform weights as the network's own initialisation, small
    random biases), float32: the GPU tests load it, this helper reads it as float64."""
    g = torch.Generator().manual_seed(seed)
    relu = math.sqrt(2.)

    def xavier(out_f, in_f, gain):
        a = gain * math.sqrt(6. / (in_f + out_f))
        return (torch.rand(out_f, in_f, generator=g) * 2 - 1) * a

    P = {}
    for li, k in enumerate((63, 256, 256, 256, 319, 256, 256)):
        P[f'mlp_feat.{li}.weight'] = xavier(256, k, relu)
    P['mlp_feat.7.weight'] = torch.cat([xavier(1, 256, 1.), xavier(256, 256, relu)])
    P['mlp_rgb.0.weight'] = xavier(128, 283, relu)
    P['mlp_rgb.1.weight'] = xavier(3, 128, 1.) * 4.            # a colour head with some contrast
    for k in list(P.keys()):
        P[k.replace('weight', 'bias')] = 0.05 * torch.randn(P[k].shape[0], generator=g)
    return P


def seeded_problem(iters, seed=SEED, n_rays=H * W):
    """-> dict: K [3,3], pose_true / base [3,4] (float64), ray_idx [iters, n_rays] int64, rand [iters, n_rays, S] float32.  The
    camera looks down +z from the origin; `base` is the true pose with PERTURBATION composed on the left."""
    g = torch.Generator().manual_seed(seed + 1000)
    K = torch.tensor([[14., 0.3, W / 2], [0., 15., H / 2], [0., 0., 1.]], dtype=f64)
    pose_true = se3_to_SE3(torch.tensor([0.1, -0.2, 0.05, 0.1, -0.05, 0.2], dtype=f64))
    base = refined_pose(torch.tensor(PERTURBATION, dtype=f64), pose_true)
    ray_idx = torch.stack([torch.randperm(H * W, generator=g)[:n_rays] for _ in range(iters)])
    rand = torch.rand(iters, n_rays, S, generator=g)
    return dict(K=K, pose_true=pose_true, base=base, ray_idx=ray_idx, rand=rand)


def reference_image(P, pose_w2c, K, n_samples=96):
    """The view of the seeded network at pose_w2c: mid-bin samples, float64 -> [H,W,3]."""
    idx = torch.arange(H * W)
    center, ray, _ = rays(pose_w2c, K, idx, W)
    with torch.no_grad():
        out = SN.render(P, center, ray, depths(torch.full((H * W, n_samples), 0.5, dtype=f64), DEPTH_RANGE), PROGRESS, BARF_C2F)
    return out['rgb'].reshape(H, W, 3)


if __name__ == '__main__':
    iters = 40
    P = {k: v.double() for k, v in seeded_params().items()}
    pb = seeded_problem(iters)
    image = reference_image(P, pb['pose_true'], pb['K'])
    hist, losses, first = loop(P, pb['base'], pb['K'], image, pb['ray_idx'], pb['rand'].double(), DEPTH_RANGE, PROGRESS, BARF_C2F)
    print('image contrast (std over pixels):', float(image.reshape(-1, 3).std(0).mean()))
    print('first gradient:', first.tolist())
    print('loss, first ten: %.6e  last ten: %.6e' % (float(losses[:10].mean()), float(losses[-10:].mean())))
    print('|se3| after %d iterations: %.4e' % (iters, float(hist[-1].norm())))
