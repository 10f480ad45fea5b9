"""Forward-only scene rendering on the GPU (pp_nerf_infer, SceneRenderer.render_view / render_rays, gen_videos):
the sample stage's outputs are pp_nerf_fwd's bits, so everything downstream is compared with torch.equal - no tolerance
anywhere except in the one comparison against the float64 oracle."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = -7.25
DEPTH_RANGE = (0.5, 3.0)


def _net(progress, seed=0, options=None, **kw):
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(**kw)
    torch.manual_seed(seed)
    net = bg_nerf.NeRF(opt, device='cuda', options=options)
    net.progress.data.fill_(progress)
    return net, opt


def _rays(R, S, seed, spread=None):
    g = torch.Generator().manual_seed(seed)
    center, ray = torch.randn(R, 3, generator=g) * 0.2, torch.randn(R, 3, generator=g)
    if spread is not None:                    # rays of very different magnitude in one batch: tile maxima != the tensor maximum
        center, ray = center * spread[:, None], ray * spread[:, None]
    depth = (torch.rand(R, S, generator=g) + torch.arange(S)) / S * 2.0 + 0.4
    return center.cuda(), ray.cuda(), depth.cuda()


def _fwd(net, center, ray, depth):
    from poseprobe_amd import ops
    R, S = depth.shape
    f = dict(dtype=torch.float32, device='cuda')
    a, _ = ops.nerf_workspace(R * S, R)
    count = torch.tensor([R * S], dtype=torch.int32, device='cuda')
    rgb, dens = torch.empty(R * S, 3, **f), torch.empty(R * S, **f)
    ops.nerf_fwd(net.flat, center, ray, depth, net.band_weights(), count, R, S, torch.empty(a, **f), rgb, dens, net.ctx)
    return rgb, dens


def _infer_guarded(net, center, ray, depth):
    """pp_nerf_infer on a workspace of exactly pp_nerf_infer_workspace floats followed by a guard region; outputs likewise."""
    from poseprobe_amd import ops
    R, S = depth.shape
    M = R * S
    f = dict(dtype=torch.float32, device='cuda')
    n = ops.nerf_infer_workspace(M, R)
    work = torch.full((n + GUARD,), PATTERN, **f)
    rgb, dens = torch.full((M * 3 + GUARD,), PATTERN, **f), torch.full((M + GUARD,), PATTERN, **f)
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    ops.nerf_infer(net.flat, center, ray, depth, net.band_weights(), count, R, S, work[:n], rgb[:M * 3], dens[:M], net.ctx)
    for name, t, used in (('work', work, n), ('rgb_samples', rgb, M * 3), ('density_samples', dens, M)):
        assert bool((t[used:] == PATTERN).all()), f'{name}: the guard behind the buffer was written'
    return rgb[:M * 3].view(M, 3), dens[:M]


# ------------------------------------------------------------------------------------------------ 1. the sample stage
@pytest.mark.parametrize('progress', [0.7, 1.0])
@pytest.mark.parametrize('R,S', [(1, 2), (1, 64), (5, 13), (3, 512), (129, 256)])
def test_infer_equals_forward_bit_for_bit(R, S, progress):
    """(1, 2) one ragged tile; (1, 64) exactly one; (5, 13) one row into the second; (3, 512) the compositing kernels' maximum S;
    (129, 256) = 516 tiles, more than 2 x 256 work-groups: a work-group walks a second tile."""
    net, _ = _net(progress, seed=S)
    center, ray, depth = _rays(R, S, seed=R + S)
    rgb, dens = _fwd(net, center, ray, depth)
    rgb_i, dens_i = _infer_guarded(net, center, ray, depth)
    assert bool(torch.isfinite(rgb).all()) and float(dens.max()) > 0
    assert torch.equal(rgb_i, rgb), f'rgb_samples differ: max {float((rgb_i - rgb).abs().max()):.3e}'
    assert torch.equal(dens_i, dens), f'density_samples differ: max {float((dens_i - dens).abs().max()):.3e}'


def test_infer_equals_forward_on_rays_of_mixed_magnitude():
    R, S = 37, 24                                       # 888 samples = 14 tiles, each within one or two rays
    spread = torch.tensor([10.0 ** ((i % 5) - 3) for i in range(R)])
    net, _ = _net(1.0, seed=3)
    center, ray, depth = _rays(R, S, seed=11, spread=spread)
    rgb, dens = _fwd(net, center, ray, depth)
    rgb_i, dens_i = _infer_guarded(net, center, ray, depth)
    assert torch.equal(rgb_i, rgb) and torch.equal(dens_i, dens)


def test_infer_matches_oracle():
    """The budgets of tests/test_hip_scene.py::test_scene_edge_shapes_match_oracle, on infer_composite's outputs."""
    from oracle import scene_nerf as SN
    R, S = 5, 65
    net, opt = _net(0.7, seed=1)
    center, ray, depth = _rays(R, S, seed=S)
    P = {k: v.detach().cpu().clone() for k, v in net.state_dict().items() if k != 'progress'}
    ref = SN.render(P, center.cpu(), ray.cpu(), depth.cpu(), 0.7, tuple(opt.barf_c2f))
    b = net.infer_composite(opt, center, ray, depth)
    for k, t in (('rgb', b.rgb), ('depth', b.d), ('opacity', b.op), ('weights', b.w), ('all_cumulated', b.cum)):
        assert_close(t.reshape(-1), ref[k].detach().reshape(-1), rtol=5e-5, atol=5e-6, name=k)


# ------------------------------------------------------------------------------------------------ 2. the workspace
def test_infer_workspace_is_at_most_225_floats_per_sample():
    from poseprobe_amd import ops
    w1, w2 = ops.nerf_infer_workspace(1000, 10), ops.nerf_infer_workspace(3000, 10)
    slope = (w2 - w1) / 2000
    fixed = w1 - slope * 1000
    assert slope <= 225 and fixed >= 0
    for M, R in ((2, 1), (64, 1), (33024, 129), (8192 * 256, 8192)):
        assert ops.nerf_infer_workspace(M, R) <= 225 * M + fixed
        assert ops.nerf_infer_workspace(M, 1) == ops.nerf_infer_workspace(M, R)
    assert ops.nerf_infer_workspace(8192 * 256, 8192) * 4 < 2 ** 31         # the default chunk's fine pass


# ------------------------------------------------------------------------------------------------ 3. other routes
@pytest.mark.parametrize('options', [{'nerf_split': 0}, {'nerf_chain': 0}], ids=lambda o: next(iter(o)))
def test_other_routes_are_refused_by_the_kernel_entry_and_served_by_the_fallback(options):
    from poseprobe_amd import _lib, bg_nerf, ops, synthetic as syn
    net, opt = _net(1.0, seed=2, options=options, sample_intvs=24)
    R, S = 8, 24
    center, ray, depth = _rays(R, S, seed=5)
    f = dict(dtype=torch.float32, device='cuda')
    work = torch.zeros(ops.nerf_infer_workspace(R * S, R), **f)
    rgb, dens = torch.zeros(R * S, 3, **f), torch.zeros(R * S, **f)
    count = torch.tensor([R * S], dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    status = _lib.lib().pp_nerf_infer(p(net.flat), p(center), p(ray), p(depth), p(net.band_weights()), p(count), R, S, p(work),
                                      p(rgb), p(dens), net.ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert status == -1, 'PP_ERR_INVALID_ARG expected'
    assert b'pp_nerf_infer' in _lib.lib().pp_last_error()
    torch.cuda.synchronize()
    assert float(rgb.abs().max()) == 0 and float(work.abs().max()) == 0, 'a refused call launched something'
    assert not net.infer_route()
    sr = bg_nerf.SceneRenderer(opt, nerf=net)
    H, W = 4, 6
    views = syn.make_views(1, H, W, seed=5)
    pose = torch.tensor(views['w2c'][:, :3, :4]).float().cuda()
    intr = torch.tensor(views['Ks']).float().cuda()
    c, r = bg_nerf.get_center_and_ray(pose, H, W, intr)
    with torch.no_grad():
        want = sr.render(opt, pose, H, W, intr, depth_range=DEPTH_RANGE, mode='val')
    got = sr.render_rays(opt, c[0], r[0], DEPTH_RANGE, mode='val', chunk_rays=H * W)
    for k in bg_nerf.VIEW_KEYS:
        assert torch.equal(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 4. whole views
@pytest.fixture(scope='module')
def scene():
    """The fixture of test_scene_render_by_slices_equals_one_pass; a coarse-only renderer and one with a fine pass that share
    the coarse network."""
    from poseprobe_amd import bg_nerf, synthetic as syn
    H, W = 12, 16
    views = syn.make_views(2, H, W, seed=5)
    pose = torch.tensor(views['w2c'][:, :3, :4]).float().cuda()
    intr = torch.tensor(views['Ks']).float().cuda()
    opt_f = bg_nerf.default_options(sample_intvs=24)
    opt_f.nerf.fine_sampling, opt_f.nerf.sample_intvs_fine = True, 24
    torch.manual_seed(9)
    fine = bg_nerf.SceneRenderer(opt_f, device='cuda')
    fine.nerf.progress.data.fill_(1.0)
    fine.nerf_fine.progress.data.fill_(1.0)
    opt_c = bg_nerf.default_options(sample_intvs=24)
    coarse = bg_nerf.SceneRenderer(opt_c, nerf=fine.nerf)
    return dict(H=H, W=W, pose=pose, intr=intr, coarse=(coarse, opt_c), fine=(fine, opt_f), slices={})


def _slices(scene, which, chunk, B):
    """render_by_slices with rand_rays = chunk: computed once per (renderer, chunk, poses) and shared."""
    key = (which, chunk, B)
    if key not in scene['slices']:
        sr, opt = scene[which]
        opt.nerf.rand_rays = chunk
        scene['slices'][key] = sr.render_by_slices(opt, scene['pose'][:B], scene['H'], scene['W'], scene['intr'][:B],
                                                   depth_range=DEPTH_RANGE, mode='val')
    return scene['slices'][key]


@pytest.mark.parametrize('which', ['coarse', 'fine'])
@pytest.mark.parametrize('chunk', [192, 100, 7])
def test_render_view_equals_render_by_slices(scene, which, chunk):
    """One chunk, a ragged second chunk, 28 chunks: identical rays, identical chunks, a bit-identical sample stage."""
    sr, opt = scene[which]
    want = _slices(scene, which, chunk, 1)
    got = sr.render_view(opt, scene['pose'][:1], scene['H'], scene['W'], scene['intr'][:1], DEPTH_RANGE, mode='val', chunk_rays=chunk)
    assert set(got.keys()) == set(want.keys()) and ('rgb_fine' in got) == (which == 'fine')
    for k in want:
        assert got[k].shape == want[k].shape, k
        assert torch.equal(got[k], want[k]), f'{k}: max difference {float((got[k] - want[k]).abs().max()):.3e}'
    assert float(got['opacity'].max()) > 0 and bool(torch.isfinite(got['rgb']).all())


def test_render_view_of_two_poses_and_refused_modes(scene):
    sr, opt = scene['fine']
    want = _slices(scene, 'fine', 100, 2)
    got = sr.render_view(opt, scene['pose'], scene['H'], scene['W'], scene['intr'], DEPTH_RANGE, mode='val', chunk_rays=100)
    assert got['rgb_fine'].shape == (2, 192, 3) and got['all_cumulated'].shape == (2, 192)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(ValueError):
        sr.render_view(opt, scene['pose'], scene['H'], scene['W'], scene['intr'], DEPTH_RANGE, mode='train')
    with pytest.raises(ValueError):
        sr.render_view(opt, scene['pose'], scene['H'], scene['W'], scene['intr'], DEPTH_RANGE, chunk_rays=0)


def test_render_view_skips_the_fine_pass_before_its_start(scene):
    sr, opt = scene['fine']
    opt.nerf.ratio_start_fine_sampling_at_x, opt.max_iter = 0.3, 1000
    try:
        early = sr.render_view(opt, scene['pose'][:1], scene['H'], scene['W'], scene['intr'][:1], DEPTH_RANGE, iter=100)
        late = sr.render_view(opt, scene['pose'][:1], scene['H'], scene['W'], scene['intr'][:1], DEPTH_RANGE, iter=300)
    finally:
        del opt.nerf['ratio_start_fine_sampling_at_x']
    assert 'rgb_fine' not in early and 'rgb_fine' in late
    assert torch.equal(early['rgb'], late['rgb'])


# ------------------------------------------------------------------------------------------------ 5. nothing else is written
def test_render_view_leaves_networks_and_pending_passes_alone(scene):
    from poseprobe_amd import bg_nerf
    sr, opt = scene['fine']
    H, W, pose, intr = scene['H'], scene['W'], scene['pose'][:1], scene['intr'][:1]
    eng = bg_nerf.SceneEngine(sr.nerf, net_fine=sr.nerf_fine)
    eng.states[0].m.fill_(0.25), eng.states[1].v.fill_(0.5), eng.states[0].grad.fill_(0.125)
    nets = (sr.nerf, sr.nerf_fine)
    state = lambda: [t.clone() for n in nets for t in (n.flat, n.progress.data)] + [t.clone() for s in eng.states for t in (s.grad, s.m, s.v)]
    params = [p for n in nets for name, p in n.named_parameters() if name != 'progress']
    idx = torch.arange(100, device='cuda')

    def pending():
        ret = sr.render(opt, pose, H, W, intr, ray_idx=idx, depth_range=DEPTH_RANGE, mode='val')
        return ret['rgb'].sum() + ret['rgb_fine'].sum()

    for n in nets:
        n.zero_grad()
    pending().backward()
    ref = [p.grad.clone() for p in params]
    for n in nets:
        n.zero_grad()
    before = state()
    loss = pending()                                               # same (R, S) as the chunks below, waiting for its backward
    sr.render_view(opt, pose, H, W, intr, DEPTH_RANGE, mode='val', chunk_rays=100)
    for a, b in zip(before, state()):
        assert torch.equal(a, b), 'render_view wrote a network, progress or optimiser state'
    loss.backward()
    for p, g0 in zip(params, ref):                                 # the weight-gradient flush uses float atomics: summation order
        assert_close(p.grad, g0.cpu(), rtol=1e-4, scaled=1e-5, name='pending pass around render_view')
    for n in nets:
        n.zero_grad()


# ------------------------------------------------------------------------------------------------ 6. held-out views
def test_evaluate_test_views_on_the_view_path(scene):
    from poseprobe_amd import evaluation, synthetic as syn
    sr, opt = scene['fine']
    H, W = scene['H'], scene['W']
    views = syn.make_views(4, H, W, seed=6)
    w2c = torch.tensor(views['w2c'][:, :3, :4]).float()
    images = torch.tensor(views['images'][3:4])
    K = torch.tensor(views['Ks'][3]).float()
    opt.nerf.rand_rays = 100
    kw = dict(refine=False)
    a = evaluation.evaluate_test_views(sr.nerf, sr.nerf_fine, opt, w2c[:3].cuda(), w2c[:3], w2c[3:4], images, K, DEPTH_RANGE, **kw)
    b = evaluation.evaluate_test_views(sr.nerf, sr.nerf_fine, opt, w2c[:3].cuda(), w2c[:3], w2c[3:4], images, K, DEPTH_RANGE,
                                       render='view', chunk_rays=100, **kw)
    assert a['table'].shape == (1, 4) and np.isfinite(a['table']).all()
    assert np.array_equal(a['table'], b['table'])
    assert tuple(b['rgbs'].shape) == (1, H, W, 3) and torch.equal(a['rgbs'], b['rgbs'])
    with pytest.raises(ValueError):
        evaluation.evaluate_test_views(sr.nerf, sr.nerf_fine, opt, w2c[:3].cuda(), w2c[:3], w2c[3:4], images, K, DEPTH_RANGE,
                                       render='rays', **kw)


# ------------------------------------------------------------------------------------------------ 7. novel views
def test_render_novel_views_frames_are_render_view_at_their_poses(scene):
    from poseprobe_amd import gen_videos, synthetic as syn
    sr, opt = scene['fine']
    H, W = scene['H'], scene['W']
    views = syn.make_views(3, H, W, seed=7)
    w2c = torch.tensor(views['w2c'][:, :3, :4]).float().cuda()
    K = torch.tensor(views['Ks']).float().cuda()
    out = gen_videos.render_novel_views(sr, opt, w2c, K, H, W, DEPTH_RANGE, dataset='dtu', n_frames=2, chunk_rays=100)
    assert tuple(out['poses_w2c'].shape) == (4, 3, 4) and tuple(out['rgb'].shape) == (4, H, W, 3) and tuple(out['depth'].shape) == (4, H, W)
    assert out['rgb'].is_cuda and out['depth'].is_cuda
    assert torch.equal(out['poses_w2c'], gen_videos.novel_view_poses(w2c, 'dtu', n_frames=2))
    for f in range(4):
        ret = sr.render_view(opt, out['poses_w2c'][f:f + 1], H, W, K[:1], DEPTH_RANGE, mode='val', chunk_rays=100)
        assert torch.equal(out['rgb'][f], ret['rgb_fine'].view(H, W, 3)), f
        assert torch.equal(out['depth'][f], ret['depth_fine'].view(H, W)), f
    assert float((out['rgb'][0] - out['rgb'][2]).abs().max()) > 0
