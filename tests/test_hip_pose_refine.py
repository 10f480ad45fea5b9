"""Test-time pose refinement on the GPU (poseprobe_amd/pose_refine.py, csrc/pp_pose_refine.hip, pp_nerf_bwd_input):
the frozen backward against the full one (bits), the two small kernels against torch / float64, one iteration and a 40-step
trajectory against the autograd route on the same kernels, the promise that nothing but the six pose numbers moves, and the
held-out-view evaluation that is built on it.  The seeded problem is tests/pose_refine_reference.py's (12 x 16 pixels, 24
samples); its reference image is rendered once, on the CPU in float64, and shared."""
import numpy as np
import pytest
import torch

from tests import pose_refine_reference as PR
from tests.helpers import assert_close, nerf_workspace_of_the_parent

pytestmark = pytest.mark.gpu

H, W, S = PR.H, PR.W, PR.S


def _net(options=None, sample_intvs=S):
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(barf_c2f=PR.BARF_C2F, sample_intvs=sample_intvs)
    net = bg_nerf.NeRF(opt, device='cuda', options=options)
    sd = dict(PR.seeded_params())
    sd['progress'] = torch.tensor(PR.PROGRESS)
    net.load_state_dict(sd)
    return net, opt


@pytest.fixture(scope='module')
def problem():
    """The seeded problem, its float64 reference image (computed once; read-only) and 40 iterations of replayed draws."""
    P64 = {k: v.double() for k, v in PR.seeded_params().items()}
    pb = PR.seeded_problem(40)
    pb['image'] = PR.reference_image(P64, pb['pose_true'], pb['K']).float()
    return pb


def _bits(t):
    return t.detach().clone().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. frozen backward = full backward
@pytest.mark.parametrize('nerf_chain', [3, 0])
@pytest.mark.parametrize('nerf_split', [1, 0])
@pytest.mark.parametrize('R,S_', [(16, 8), (37, 200), (96, 40), (1, 2)])
def test_frozen_backward_gives_the_bits_of_the_full_backward(R, S_, nerf_split, nerf_chain):
    """pp_nerf_bwd_input issues pp_nerf_bwd's launches minus the nine weight-gradient products: the same kernels read the same
    bytes and every sum on the way to the rays is order-free, so g_center and g_ray are EQUAL - no tolerance.  No parameter
    gradient is touched: a canary-filled gradient block of a live SceneEngine on the same network keeps its bits, and the
    workspace sizes are the parent's."""
    from poseprobe_amd import bg_nerf, ops
    net, opt = _net(options={'nerf_split': nerf_split, 'nerf_chain': nerf_chain}, sample_intvs=S_)
    eng = bg_nerf.SceneEngine(net)
    eng.grad.fill_(-7.25)
    canary = torch.full_like(net.flat, 3.5)
    M = R * S_
    assert ops.nerf_workspace(M, R) == nerf_workspace_of_the_parent(M, R)
    g = torch.Generator().manual_seed(R * 1000 + S_)
    center = (torch.randn(R, 3, generator=g) * 0.3).cuda()
    ray = (torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * (0.7 + torch.rand(R, 1, generator=g))).cuda()
    depth = ((torch.rand(R, S_, generator=g) + torch.arange(S_)) / S_ * 2.0 + 0.4).cuda().contiguous()
    g_rgb_s, g_dens = torch.randn(M, 3, generator=g).cuda(), torch.randn(M, generator=g).cuda()
    n_acts, n_scr = ops.nerf_workspace(M, R)
    f = dict(dtype=torch.float32, device='cuda')
    acts, count = torch.empty(n_acts, **f), torch.tensor([M], dtype=torch.int32, device='cuda')
    rgb_s, dens = torch.empty(M, 3, **f), torch.empty(M, **f)
    ops.nerf_fwd(net.flat, center, ray, depth, net.band_weights(), count, R, S_, acts, rgb_s, dens, net.ctx)
    flat0 = _bits(net.flat)
    pgrad = torch.zeros_like(net.flat)
    gc_full, gr_full = torch.empty(R, 3, **f), torch.empty(R, 3, **f)
    ops.nerf_bwd(net.flat, ray, depth, count, R, S_, acts, rgb_s, g_rgb_s, g_dens, torch.zeros(n_scr, **f), pgrad, gc_full, gr_full, net.ctx)
    gc_in, gr_in = torch.full((R, 3), float('nan'), **f), torch.full((R, 3), float('nan'), **f)
    ops.nerf_bwd_input(net.flat, ray, depth, count, R, S_, acts, rgb_s, g_rgb_s, g_dens, torch.zeros(n_scr, **f), gc_in, gr_in, net.ctx)
    torch.cuda.synchronize()
    assert float(pgrad.abs().max()) > 0 and float(gr_full.abs().max()) > 0 and bool(torch.isfinite(gr_full).all())
    assert torch.equal(_bits(gc_in), _bits(gc_full)), 'g_center differs from the full backward'
    assert torch.equal(_bits(gr_in), _bits(gr_full)), 'g_ray differs from the full backward'
    assert bool((eng.grad == -7.25).all()) and bool((canary == 3.5).all()) and torch.equal(_bits(net.flat), flat0)
    # the wrapper follows its neighbours: host tensors are refused
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.nerf_bwd_input(net.flat, ray.cpu(), depth, count, R, S_, acts, rgb_s, g_rgb_s, g_dens, torch.zeros(n_scr, **f), gc_in, gr_in)
    with pytest.raises(RuntimeError, match='needs'):
        ops.nerf_bwd_input(net.flat, ray, depth, count, R, S_, acts, rgb_s, g_rgb_s, g_dens, torch.zeros(n_scr - 1, **f), gc_in, gr_in)


# ------------------------------------------------------------------------------------------------ 2. rays kernel
@pytest.mark.parametrize('idx', [[0], [34], [0, 34] + [(11 * i + 3) % 35 for i in range(35)]], ids=['first', 'last', '37'])
def test_rays_kernel_equals_the_torch_camera_algebra(idx):
    """pp_nerf_rays_select on a 5 x 7 image with a skewed K against bg_nerf.get_center_and_ray (K.inverse(), cam2world) at the
    same pixels: targets equal, geometry within the budget test_scene_pose_gradient_through_torch_camera_chain uses for it."""
    from poseprobe_amd import bg_nerf, camera, ops
    h, w = 5, 7
    g = torch.Generator().manual_seed(11)
    K = torch.tensor([[6.5, 0.4, 3.3], [0., 7.25, 2.6], [0., 0., 1.]]).cuda()
    w2c = PR.se3_to_SE3(torch.tensor([0.3, -0.5, 0.2, 0.4, -0.3, 1.1], dtype=torch.float64)).float().cuda()
    image = torch.rand(h, w, 3, generator=g).cuda()
    ray_idx = torch.tensor(idx, dtype=torch.int32).cuda()
    N = len(idx)
    assert N in (1, 37)
    f = dict(dtype=torch.float32, device='cuda')
    center, ray, dir_cam, target = (torch.full((N, 3), float('nan'), **f) for _ in range(4))
    c2w = camera.pose.invert(w2c).contiguous()
    ops.nerf_rays_select(c2w, K, ray_idx, h, w, image, center, ray, dir_cam, target)
    c_ref, r_ref = bg_nerf.get_center_and_ray(w2c[None], h, w, K[None])
    sel = ray_idx.long()
    assert torch.equal(target, image.view(-1, 3)[sel])
    assert_close(center, c_ref[0, sel], rtol=1e-5, atol=1e-6, name='center')
    assert_close(ray, r_ref[0, sel], rtol=1e-5, atol=1e-6, name='ray')
    x, y = (sel % w).float() + 0.5, (sel // w).float() + 0.5
    d_ref = torch.stack([x, y, torch.ones_like(x)], dim=-1).double() @ K.double().inverse().T
    assert_close(dir_cam, d_ref, rtol=1e-5, atol=1e-6, name='dir_cam')
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.nerf_rays_select(c2w.cpu(), K, ray_idx, h, w, image, center, ray, dir_cam, target)
    with pytest.raises(RuntimeError, match='needs'):
        ops.nerf_rays_select(c2w, K, ray_idx, h, w, image, center[:N - 1] if N > 1 else center[:0], ray, dir_cam, target)


# ------------------------------------------------------------------------------------------------ 3. MSE kernel
@pytest.mark.parametrize('n', [3, 3 * 1025])
def test_mse_kernel_equals_float64_and_repeats_its_bits(n):
    """pp_nerf_mse_loss against float64 on the same float32 inputs, the budget of its twin (test_photometric_loss_kernel_equals_
    torch_huber: loss 2e-6, gradient 1e-6 relative); one ray, and a length beyond the 1024-thread stride; two runs, same bits."""
    from poseprobe_amd import ops
    g = torch.Generator().manual_seed(5 + n)
    pred, label = (torch.rand(n, generator=g) * 2.0 - 0.5).cuda(), torch.rand(n, generator=g).cuda()
    p64 = pred.double().requires_grad_(True)
    ref = 0.75 * torch.nn.functional.mse_loss(p64, label.double())
    ref.backward()
    out = []
    for _ in range(2):
        loss, gp = torch.full((1,), float('nan'), device='cuda'), torch.full((n,), float('nan'), device='cuda')
        ops.nerf_mse_loss(pred, label, 0.75, loss, gp)
        out.append((loss, gp))
    assert_close(out[0][0][0], ref.detach(), rtol=2e-6, name=f'mse[{n}]')
    assert_close(out[0][1], p64.grad, rtol=1e-6, atol=1e-12, name=f'mse grad[{n}]')
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.nerf_mse_loss(pred.cpu(), label, 1.0, out[0][0], out[0][1])


# ------------------------------------------------------------------------------------------------ 4. one iteration
def _twin_loss(sr, opt, net, se3, pb, it, rays64=False):
    """The autograd route on the same kernels: camera.current_pose_c2w -> SceneRenderer.render(mode = 'test-optim') -> mse_loss.
    rays64: the rays formed in float64 from the float32 pose and rounded (the second twin of the trajectory test)."""
    from poseprobe_amd import bg_nerf, camera
    base, K = pb['base'].float().cuda(), pb['K'].float().cuda()
    idx, rand = pb['ray_idx'][it].cuda(), pb['rand'][it].cuda()[None, :, :, None]
    image = pb['image'].cuda()
    w2c, _ = camera.current_pose_c2w(se3, base[None], fix_first=False)
    if not rays64:
        pred = sr.render(opt, w2c, H, W, K[None], ray_idx=idx, depth_range=PR.DEPTH_RANGE, mode='test-optim', rand=[rand])
    else:
        pix = torch.stack([(idx % W).double() + 0.5, (idx // W).double() + 0.5], dim=-1)
        center, ray = bg_nerf.get_center_and_ray_at_pixels(w2c.double(), pix, pb['K'].cuda()[None])
        center, ray = center.float(), ray.float()
        jitter = rand + torch.arange(S, device='cuda')[None, None, :, None].float()
        depth = jitter / S * (PR.DEPTH_RANGE[1] - PR.DEPTH_RANGE[0]) + PR.DEPTH_RANGE[0]
        pred = net.composite(opt, ray, net.forward_samples(opt, center, ray, depth, mode='test-optim'), depth)
    return torch.nn.functional.mse_loss(pred['rgb'][0], image.view(-1, 3)[idx])


def _replay(pb, iters):
    return dict(ray_idx=pb['ray_idx'][:iters], depth_rand=pb['rand'][:iters])


def test_one_iteration_matches_the_autograd_route(problem):
    """refine(iters = 1) on all 192 pixels: the first gradient against autograd through the same kernels (the budget of
    test_scene_pose_gradient_through_torch_camera_chain for this quantity: the rays' gradients cancel down to the pose's), the
    loss, Adam's first step, and the returned pose = compose([se3_to_SE3(se3), base])."""
    from poseprobe_amd import bg_nerf, camera, pose_refine
    pb = problem
    net, opt = _net()
    sr = bg_nerf.SceneRenderer(opt, nerf=net)
    se3 = torch.zeros(1, 6, device='cuda', requires_grad=True)
    loss = _twin_loss(sr, opt, net, se3, pb, 0)
    loss.backward()
    refiner = pose_refine.PoseRefiner(net, opt, H, W, pb['K'], PR.DEPTH_RANGE, rand_rays=H * W)
    assert refiner.N == H * W
    out = refiner.refine(pb['base'], pb['image'], iters=1, replay=_replay(pb, 1))
    assert tuple(out['pose_w2c'].shape) == (3, 4) and tuple(out['se3'].shape) == (6,) and tuple(out['losses'].shape) == (1,)
    print('se3_grad_first', out['se3_grad_first'].tolist(), 'autograd', se3.grad[0].tolist())
    assert_close(out['se3_grad_first'], se3.grad[0], rtol=1e-3, scaled=1e-2, name='se3 gradient')
    # the two routes round the rays differently (closed-form K^-1 and R d here, K.inverse() and (R d + t) - t there: ~1e-7
    # relative); the highest open band (2^5 pi at this progress) turns that into ~1e-5 of a colour, and a colour error e moves
    # mean(d^2) with |d| ~ 0.06 by at most 2 e / |d| = 3e-4 relative if every ray erred the same way
    assert_close(out['losses'][0], loss.detach(), rtol=5e-4, name='loss')
    assert_close(out['se3'], -5e-4 * torch.sign(out['se3_grad_first']), rtol=1e-4, name="Adam's first step")
    want = camera.pose.compose([camera.lie.se3_to_SE3(out['se3'][None])[0], pb['base'].float().cuda()])
    assert_close(out['pose_w2c'], want, rtol=1e-5, atol=1e-6, name='pose = compose([se3_to_SE3(se3), base])')
    assert_close(out['pose_w2c'], PR.refined_pose(out['se3'].double().cpu(), pb['base']), rtol=1e-5, atol=1e-6, name='pose (float64)')


# ------------------------------------------------------------------------------------------------ 5. trajectory
def test_trajectory_follows_the_autograd_twin(problem):
    """40 iterations with replayed draws; se3 after every tenth against the autograd twin (torch.optim.Adam on the route of
    _twin_loss).  The tolerance is measured, not chosen: a second twin forms its rays in float64 and rounds them - the same
    mathematics, another float32 rounding of the rays - and the largest difference between the twins, relative to the distance
    se3 has moved, is the floor; the HIP loop may differ from the first twin by 4 x that floor (the project's usual margin over
    what the reference loses by itself).  Figures are printed before they are asserted.
    Condition on the inputs: the twin's loss falls (mean of the last ten iterations below the first ten), as
    `python tests/pose_refine_reference.py` shows for the seed in float64: 3.95e-3 -> 3.55e-3."""
    from poseprobe_amd import bg_nerf, pose_refine
    pb = problem
    net, opt = _net()
    sr = bg_nerf.SceneRenderer(opt, nerf=net)

    def twin(rays64):
        se3 = torch.zeros(1, 6, device='cuda', requires_grad=True)
        optim = torch.optim.Adam([se3], lr=5e-4)
        marks, losses = [], []
        for it in range(40):
            optim.zero_grad()
            loss = _twin_loss(sr, opt, net, se3, pb, it, rays64)
            loss.backward()
            optim.step()
            losses.append(loss.detach())
            if it % 10 == 9:
                marks.append(se3.detach()[0].double().clone())
        return torch.stack(marks), torch.stack(losses)

    a, losses = twin(False)
    b, _ = twin(True)
    first, last = float(losses[:10].mean()), float(losses[-10:].mean())
    print(f'twin loss: first ten {first:.4e}, last ten {last:.4e}')
    assert last < first, 'the seeded problem does not optimise: the comparison would say nothing'
    moved = a.norm(dim=1)
    floor = float(((a - b).abs().amax(dim=1) / moved).max())
    refiner = pose_refine.PoseRefiner(net, opt, H, W, pb['K'], PR.DEPTH_RANGE, rand_rays=H * W)
    hip = torch.stack([refiner.refine(pb['base'], pb['image'], iters=n, replay=_replay(pb, n))['se3'].double() for n in (10, 20, 30, 40)])
    dev = float(((hip - a).abs().amax(dim=1) / moved).max())
    print(f'floor (twin against float64-ray twin, relative to |se3|): {floor:.3e}; HIP loop against the twin: {dev:.3e}; '
          f'|se3| at 10..40: {moved.tolist()}')
    assert floor > 0
    assert dev <= 4 * floor, f'HIP loop deviates {dev:.3e} of the distance moved, floor {floor:.3e}'


# ------------------------------------------------------------------------------------------------ 6. nothing else moves
def test_refinement_moves_nothing_but_the_pose(problem):
    """net.flat, a sharing SceneEngine's grad / m / v and its counters keep their bits across refine() - with a deterministic
    engine, whose ordered-flush workspace is attached to the network's context and simply not used by the frozen backward - and
    the training step taken afterwards equals, bit for bit, the step of a twin engine that saw no refinement."""
    from poseprobe_amd import bg_nerf, pose_refine
    pb = problem
    g = torch.Generator().manual_seed(9)
    R = 64
    center, ray = (torch.randn(R, 3, generator=g) * 0.3).cuda(), torch.randn(R, 3, generator=g).cuda()
    depth = ((torch.rand(R, S, generator=g) + torch.arange(S)) / S * 2.0 + 0.4).cuda().contiguous()
    image = torch.rand(R, 3, generator=g).cuda()
    state = lambda e, n: {k: _bits(t) for k, t in (('flat', n.flat), ('grad', e.grad), ('m', e.m), ('v', e.v))}
    results = []
    for refine in (True, False):
        net, opt = _net()
        eng = bg_nerf.SceneEngine(net, deterministic=True)
        eng.step(center, ray, depth, image)                       # moments and counters that are not trivially zero
        eng.grad.fill_(0.125)                                     # a pending gradient block
        flags = [p.requires_grad for p in net.parameters()]
        before, counters = state(eng, net), (eng.step_count, eng.states[0].steps, eng.states[0].has_grad)
        if refine:
            refiner = pose_refine.PoseRefiner(net, opt, H, W, pb['K'], PR.DEPTH_RANGE, rand_rays=100)
            out = refiner.refine(pb['base'], pb['image'], iters=3, generator=torch.Generator(device='cuda').manual_seed(1))
            assert bool(torch.isfinite(out['losses']).all()) and float(out['se3'].abs().max()) > 0
            after = state(eng, net)
            for k in before:
                assert torch.equal(before[k], after[k]), f'{k} changed during refine()'
            assert counters == (eng.step_count, eng.states[0].steps, eng.states[0].has_grad)
            assert flags == [p.requires_grad for p in net.parameters()]
        eng.grad.zero_()
        eng.step(center, ray, depth, image)
        results.append(state(eng, net))
    for k in results[0]:
        assert torch.equal(results[0][k], results[1][k]), f'{k}: the step after a refinement differs from the step without one'


# ------------------------------------------------------------------------------------------------ 7. held-out views
def test_evaluate_test_views_scores_three_views(problem):
    from poseprobe_amd import bg_nerf, evaluation
    pb = problem
    net, opt = _net()
    t = lambda v: torch.tensor(v, dtype=torch.float64)
    GT_train = torch.stack([PR.se3_to_SE3(t(v)) for v in ([0.1, -0.2, 0.05, 0.1, -0.05, 0.2], [0.0, 0.2, 0.1, -0.4, 0.1, 0.3],
                                                          [-0.2, 0.1, 0.0, 0.3, 0.2, 0.1])])
    # the optimised poses: the ground truth seen from a frame that is rotated, shifted and 1.3 times smaller
    Rs, ts, s = PR.se3_to_SE3(t([0.2, 0.1, -0.3, 0, 0, 0]))[:, :3], t([0.1, -0.2, 0.05]), 1.3
    train = torch.stack([PR.backtrack(p, Rs, ts, s) for p in GT_train]).float().cuda()
    GT_test = torch.stack([PR.se3_to_SE3(t(v)) for v in ([0.05, -0.1, 0.0, 0.0, 0.05, 0.2], [0.1, 0.1, 0.05, -0.2, 0.0, 0.25],
                                                         [-0.1, 0.0, 0.1, 0.1, 0.1, 0.15])]).float().cuda()
    images = torch.rand(3, H, W, 3, generator=torch.Generator().manual_seed(2)) * 0.2 + pb['image'][None] * 0.8
    K = pb['K'].float()
    plain = evaluation.evaluate_test_views(net, None, opt, train, GT_train.float(), GT_test, images, K, PR.DEPTH_RANGE, refine=False)
    assert plain['table'].shape == (3, 4) and tuple(plain['poses_w2c'].shape) == (3, 3, 4) and plain['losses'] is None
    # the alignment recovers the Sim(3) (rotation_distance clamps at acos(1 - 1e-7) = 0.026 degrees)
    assert float(plain['error'].R.max()) < 0.05 and float(plain['error'].t.max()) < 1e-2
    base = evaluation.backtrack_from_aligning_the_trajectory(GT_test, plain['sim3']).float().cuda()
    assert_close(plain['poses_w2c'], base, rtol=0, atol=0, name='backtracked poses')
    sr = bg_nerf.SceneRenderer(opt, nerf=net)
    keys = ('psnr', 'psnr_fore', 'psnr_back', 'ssim')
    for i in range(3):
        rgb = sr.render_by_slices(opt, base[i:i + 1], H, W, K.cuda()[None], PR.DEPTH_RANGE, mode='val')['rgb'].view(H, W, 3)
        m = evaluation.image_metrics(rgb, images[i])
        assert_close(plain['table'][i], torch.stack([m[k] for k in keys]), rtol=1e-6, atol=1e-6, name=f'view {i}')
    out = evaluation.evaluate_test_views(net, None, opt, train, GT_train.float(), GT_test, images, K, PR.DEPTH_RANGE, refine=True,
                                         iters=3, rand_rays=64, generator=torch.Generator(device='cuda').manual_seed(3))
    assert out['table'].shape == (3, 4) and tuple(out['poses_w2c'].shape) == (3, 3, 4) and tuple(out['losses'].shape) == (3, 3)
    assert bool(torch.isfinite(out['losses']).all()) and np.isfinite(out['table']).all()
    assert float((out['poses_w2c'] - base).abs().max()) > 0
