"""Test-time pose refinement, the parts that need no GPU: the wrapper's refusals fire before anything is uploaded (the network
here is a stand-in without a device), and the float64 helper (tests/pose_refine_reference.py) composes the held-out pose in
eval.py's order - checked against 4 x 4 matrix algebra written out here and against the product's own pose functions."""
import types

import numpy as np
import pytest
import torch

from tests import pose_refine_reference as PR


def _refiner(K=None, **kw):
    from poseprobe_amd import bg_nerf, pose_refine
    opt = bg_nerf.default_options(sample_intvs=4)
    net = types.SimpleNamespace(opt=opt)                      # no `flat`: touching the device would raise AttributeError
    K = torch.tensor([[10., 0.5, 3.5], [0., 11., 2.5], [0., 0., 1.]]) if K is None else K
    return pose_refine.PoseRefiner(net, opt, 5, 7, K, (0.5, 3.0), **kw)


@pytest.mark.parametrize('entry,value', [((1, 0), 0.1), ((2, 0), 1e-3), ((2, 1), -2.), ((2, 2), 0.5), ((0, 0), 0.)])
def test_intrinsics_outside_the_closed_form_are_refused(entry, value):
    K = torch.tensor([[10., 0.5, 3.5], [0., 11., 2.5], [0., 0., 1.]])
    K[entry] = value
    with pytest.raises(ValueError, match='upper-triangular'):
        _refiner(K)
    with pytest.raises(ValueError, match=r'\[3,3\]'):
        _refiner(torch.eye(4))
    r = _refiner()
    with pytest.raises(ValueError, match='upper-triangular'):
        r.set_intrinsics(K)


def test_refine_refuses_bad_arguments_before_any_upload():
    r = _refiner(rand_rays=6)
    assert r.N == 6 and _refiner().N == 35                   # default rand_rays = 1024, capped at H * W
    base, image = torch.eye(3, 4), torch.zeros(5, 7, 3)
    with pytest.raises(ValueError, match='iters'):
        r.refine(base, image, iters=0)
    with pytest.raises(ValueError, match='image'):
        r.refine(base, torch.zeros(7, 5, 3), iters=2)
    with pytest.raises(ValueError, match='base_w2c'):
        r.refine(torch.eye(4), image, iters=2)
    rand = torch.rand(2, 6, 4)
    for bad in (35, -1):
        idx = torch.zeros(2, 6, dtype=torch.int64)
        idx[1, 3] = bad
        with pytest.raises(ValueError, match='outside'):
            r.refine(base, image, iters=2, replay=dict(ray_idx=idx, depth_rand=rand))
    with pytest.raises(ValueError, match='replay'):
        r.refine(base, image, iters=3, replay=dict(ray_idx=torch.zeros(2, 6, dtype=torch.int64), depth_rand=rand))
    with pytest.raises(ValueError, match='integer'):
        r.refine(base, image, iters=2, replay=dict(ray_idx=torch.zeros(2, 6), depth_rand=rand))
    # in range: the checks pass and the first touch of the device is reached (the stand-in has none)
    with pytest.raises(AttributeError):
        r.refine(base, image, iters=2, replay=dict(ray_idx=torch.full((2, 6), 34), depth_rand=rand))


def _hom(p):
    return np.vstack([np.asarray(p, dtype=np.float64), [0., 0., 0., 1.]])


def _rodrigues(w):
    th = np.linalg.norm(w)
    k = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    return np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * k @ k


def test_helper_composes_the_held_out_pose_in_the_reference_order():
    """A hand-made case: GT pose, a Sim(3) (R_s, t_s, s) that maps the optimised camera-to-world poses onto the ground truth, and
    a pure-rotation / pure-translation correction.  Expected, in 4 x 4 matrices: c2w_rec = [R_s^T R_gt | R_s^T (c_gt - t_s) / s],
    pose = inv(c2w_rec) applied AFTER the correction (x_cam = M_base M_refine x)."""
    Rg, Rs = _rodrigues(np.array([0.3, -0.2, 0.5])), _rodrigues(np.array([-0.4, 0.1, 0.2]))
    GT = np.hstack([Rg, [[0.2], [-0.1], [1.5]]])
    ts, s = np.array([0.3, 0.2, -0.1]), 1.7
    c2w = np.linalg.inv(_hom(GT))
    rec = np.eye(4)
    rec[:3, :3], rec[:3, 3] = Rs.T @ c2w[:3, :3], Rs.T @ (c2w[:3, 3] - ts) / s
    base = np.linalg.inv(rec)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    got = PR.backtrack(t(GT), t(Rs), t(ts), s)
    np.testing.assert_allclose(got.numpy(), base[:3], rtol=0, atol=1e-14)
    # the product's backtrack on the same numbers
    from poseprobe_amd import camera, evaluation
    from poseprobe_amd.losses import _AttrDict
    sim3 = _AttrDict(R=t(Rs)[None], t=t(ts).reshape(1, 3, 1), s=s, type='traj_align')
    np.testing.assert_allclose(evaluation.backtrack_from_aligning_the_trajectory(t(GT)[None], sim3)[0].numpy(), base[:3], rtol=0, atol=1e-14)
    # pure rotation, then pure translation: se3_to_SE3 = [exp(w^) | 0] and [I | u]
    w = np.array([0.2, 0.3, -0.1])
    Mr = np.eye(4)
    Mr[:3, :3] = _rodrigues(w)
    pose = PR.held_out_pose(t(np.concatenate([w, np.zeros(3)])), t(GT), t(Rs), t(ts), s)
    np.testing.assert_allclose(pose.numpy(), (base @ Mr)[:3], rtol=0, atol=1e-13)
    u = np.array([0.05, -0.2, 0.1])
    Mt = np.eye(4)
    Mt[:3, 3] = u
    pose = PR.held_out_pose(t(np.concatenate([np.zeros(3), u])), t(GT), t(Rs), t(ts), s)
    np.testing.assert_allclose(pose.numpy(), (base @ Mt)[:3], rtol=0, atol=1e-14)
    # the product's compose (float32 by construction of camera.pose) agrees with the helper's order
    both = t(np.concatenate([w, u]))
    want = PR.held_out_pose(both, t(GT), t(Rs), t(ts), s)
    got = camera.pose.compose([PR.se3_to_SE3(both), t(base[:3])])
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=5e-7)
    # inversion round trip and the rays of the helper: the centre is the camera position, dir_cam = K^-1 [x, y, 1]
    K = t([[10., 0.5, 3.5], [0., 11., 2.5], [0., 0., 1.]])
    center, ray, d = PR.rays(want, K, torch.tensor([0, 34]), 7)
    np.testing.assert_allclose(center[0].numpy(), np.linalg.inv(_hom(want.numpy()))[:3, 3], rtol=0, atol=1e-14)
    np.testing.assert_allclose((K @ d[1]).numpy(), [6.5, 4.5, 1.], rtol=0, atol=1e-13)
    np.testing.assert_allclose(ray.numpy(), (d @ want[:, :3]).numpy(), rtol=0, atol=1e-14)


def test_helper_loop_starts_from_zero_and_takes_sign_steps():
    """Adam's first update is lr * sign(gradient): the loop's first row pins the optimiser wiring (zero start, fresh state)."""
    P = {k: v.double() for k, v in PR.seeded_params().items()}
    pb = PR.seeded_problem(2, n_rays=24)
    image = torch.rand(PR.H, PR.W, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    hist, losses, first = PR.loop(P, pb['base'], pb['K'], image, pb['ray_idx'], pb['rand'].double(), PR.DEPTH_RANGE, PR.PROGRESS,
                                  PR.BARF_C2F)
    assert hist.shape == (2, 6) and losses.shape == (2,) and bool((first != 0).all())
    np.testing.assert_allclose(hist[0].numpy(), (-5e-4 * torch.sign(first)).numpy(), rtol=1e-6, atol=0)
    se3 = torch.zeros(6, dtype=torch.float64)
    l0 = PR.iteration_loss(P, se3, pb['base'], pb['K'], image, pb['ray_idx'][0], pb['rand'][0].double(), PR.DEPTH_RANGE, PR.PROGRESS,
                           PR.BARF_C2F)
    assert float(l0) == float(losses[0])
