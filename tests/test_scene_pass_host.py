"""CPU-only checks of the scene branch's small host helpers: bg_nerf.stratified_depths against the four expressions it replaced,
bit for bit, and SceneRenderer._fine_active against its truth table."""
import itertools

import pytest
import torch

RANGE = (0.5, 3.0)


def _opt(param):
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(sample_intvs=8)
    opt.nerf.depth.param = param
    return opt


def _param_map(opt, depth):
    return {'metric': depth, 'inverse': 1 / (depth + 1e-8)}[opt.nerf.depth.param]


# the expressions as they stood at their four sites, op for op
def _was_sample_depth(opt, rand, depth_range):                       # bg_nerf.sample_depth, [B, N, S, 1]
    depth_min, depth_max = depth_range
    n_samples = rand.shape[2]
    rand = rand + torch.arange(n_samples)[None, None, :, None].float()
    depth = rand / n_samples * (depth_max - depth_min) + depth_min
    return _param_map(opt, depth)


def _was_render_replay(opt, rand, depth_range):                      # SceneRenderer.render, [B, N, S, 1]
    S = rand.shape[2]
    jitter = rand + torch.arange(S)[None, None, :, None].float()
    depth = jitter / S * (depth_range[1] - depth_range[0]) + depth_range[0]
    return _param_map(opt, depth)


def _was_joint_replay(opt, rand, depth_range):                       # joint.DualBranchEngine.forward_backward, twice; no param map
    S = rand.shape[2]
    jit = rand + torch.arange(S)[None, None, :, None].float()
    return jit / S * (depth_range[1] - depth_range[0]) + depth_range[0]


def _was_depths_from_rand(opt, rand, depth_range):                   # pose_refine.depths_from_rand, [..., S]
    S = rand.shape[-1]
    jitter = rand + torch.arange(S).float()
    depth = jitter / S * (depth_range[1] - depth_range[0]) + depth_range[0]
    return _param_map(opt, depth)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('param', ['metric', 'inverse'])
@pytest.mark.parametrize('draw', ['half', 'random'])
def test_stratified_depths_equals_the_expressions_it_replaced(param, draw):
    from poseprobe_amd import bg_nerf
    opt = _opt(param)
    g = torch.Generator().manual_seed(11)
    for shape in ((2, 5, 8, 1), (5, 8)):
        rand = 0.5 * torch.ones(*shape) if draw == 'half' else torch.rand(*shape, generator=g)
        got = bg_nerf.stratified_depths(opt, rand, RANGE)
        if len(shape) == 4:
            assert _same_bits(got, _was_sample_depth(opt, rand, RANGE))
            assert _same_bits(got, _was_render_replay(opt, rand, RANGE))
            if param == 'metric':                     # joint.py left the map out: for 'inverse' its replayed draws change
                assert _same_bits(got, _was_joint_replay(opt, rand, RANGE))
            else:
                assert _same_bits(got, _param_map(opt, _was_joint_replay(opt, rand, RANGE)))
            # the [..., S] layout of the same draws gives the same numbers
            assert _same_bits(bg_nerf.stratified_depths(opt, rand[..., 0], RANGE), got[..., 0])
        else:
            assert _same_bits(got, _was_depths_from_rand(opt, rand, RANGE))
        lo, hi = (RANGE if param == 'metric' else (1 / (RANGE[1] + 1e-8), 1 / (RANGE[0] + 1e-8)))
        assert float(got.min()) >= lo - 1e-6 and float(got.max()) <= hi + 1e-6


def test_sample_depth_goes_through_the_helper():
    """A fresh draw and a replay of the same draw agree bit for bit, for both depth parametrisations."""
    from poseprobe_amd import bg_nerf
    for param in ('metric', 'inverse'):
        opt = _opt(param)
        fresh = bg_nerf.sample_depth(opt, 2, 5, 8, RANGE, mode='train', device='cpu', generator=torch.Generator().manual_seed(3))
        rand = torch.rand(2, 5, 8, 1, generator=torch.Generator().manual_seed(3))
        assert _same_bits(fresh, bg_nerf.stratified_depths(opt, rand, RANGE))
        mid = bg_nerf.sample_depth(opt, 2, 5, 8, RANGE, mode='val', device='cpu')
        assert _same_bits(mid, bg_nerf.stratified_depths(opt, 0.5 * torch.ones(2, 5, 8, 1), RANGE))


def test_fine_active_truth_table():
    from poseprobe_amd import bg_nerf
    max_iter = 1000
    for fine_sampling, start, it in itertools.product((False, True), (None, 0.3), (None, 299, 300, 301)):
        opt = bg_nerf.default_options()
        opt.max_iter = max_iter
        opt.nerf.fine_sampling = fine_sampling
        if start is not None:
            opt.nerf.ratio_start_fine_sampling_at_x = start
        # active = switched on, and not (a start and an iteration are both given and the iteration lies before the start)
        want = fine_sampling and not (start is not None and it is not None and it < 300)
        got = bg_nerf.SceneRenderer._fine_active(opt, it)
        assert got is want, (fine_sampling, start, it)
    opt = bg_nerf.default_options()
    opt.nerf.fine_sampling, opt.nerf.ratio_start_fine_sampling_at_x, opt.max_iter = True, None, max_iter
    assert bg_nerf.SceneRenderer._fine_active(opt, 0) is True          # the attribute present but None: no start
