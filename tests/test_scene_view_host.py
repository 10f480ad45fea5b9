"""Host side of forward-only scene rendering and the novel-view pose paths (no GPU): chunk planning, argument checks that come
before any device work, and poseprobe_amd.gen_videos / camera.get_novel_view_poses against the recorded run of the reference's own
functions (tests/golden/novel_view_poses.npz, written by tools/make_novel_views_golden.py; inputs: tests/novel_views_reference.py)."""

import numpy as np
import pytest
import torch

from tests import novel_views_reference as R
from tests.helpers import load


# ------------------------------------------------------------------------------------------------ chunks
def test_plan_chunks():
    from poseprobe_amd.bg_nerf import plan_chunks
    assert plan_chunks(192, 192) == [(0, 192)]
    assert plan_chunks(192, 100) == [(0, 100), (100, 92)]                     # ragged last chunk
    assert plan_chunks(192, 8192) == [(0, 192)]                               # chunk_rays > H * W
    assert plan_chunks(15, 7) == [(0, 7), (7, 7), (14, 1)]
    p = plan_chunks(1200 * 1600, 8192)
    assert len(p) == 235 and sum(n for _, n in p) == 1200 * 1600 and p[-1] == (234 * 8192, 1200 * 1600 - 234 * 8192)
    assert all(c == i * 8192 for i, (c, _) in enumerate(p))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            plan_chunks(192, bad)
    with pytest.raises(ValueError):
        plan_chunks(0, 8)


class _NoDevice:
    """Stands where a network would: any use of it is device work that should not have been reached."""

    flat = torch.zeros(1)

    def __getattr__(self, name):
        raise AssertionError(f'the network was used ({name}) before the arguments were checked')


def test_argument_checks_come_before_any_device_work():
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(sample_intvs=8)
    sr = bg_nerf.SceneRenderer(opt, nerf=_NoDevice(), nerf_fine=None)
    pose, intr = torch.eye(3, 4)[None], torch.eye(3)[None]
    rays = torch.zeros(5, 3)
    for mode in ('train', 'test-optim', None):
        with pytest.raises(ValueError, match='mode'):
            sr.render_view(opt, pose, 4, 4, intr, (0.5, 3.0), mode=mode)
        with pytest.raises(ValueError, match='mode'):
            sr.render_rays(opt, rays, rays, (0.5, 3.0), mode=mode)
    with pytest.raises(ValueError, match='chunk_rays'):
        sr.render_view(opt, pose, 4, 4, intr, (0.5, 3.0), chunk_rays=0)
    with pytest.raises(ValueError, match='chunk_rays'):
        sr.render_rays(opt, rays, rays, (0.5, 3.0), chunk_rays=-3)
    with pytest.raises(ValueError):
        sr.render_view(opt, torch.eye(4)[None], 4, 4, intr, (0.5, 3.0))          # [B,4,4] is not a pose
    with pytest.raises(ValueError):
        sr.render_rays(opt, rays, torch.zeros(4, 3), (0.5, 3.0))


def test_evaluate_test_views_refuses_an_unknown_render_path_first():
    from poseprobe_amd import bg_nerf, evaluation
    with pytest.raises(ValueError, match='render'):
        evaluation.evaluate_test_views(_NoDevice(), None, bg_nerf.default_options(), None, None, None, None, None, (0.5, 3.0),
                                       render='tiles')


# ------------------------------------------------------------------------------------------------ pose paths
@pytest.fixture(scope='module')
def golden():
    return load('novel_view_poses.npz')


def _spread(golden, quantity):
    return max(float(np.abs(golden[f'{quantity}.{c["name"]}'] - golden[f'{quantity}.{c["name"]}.f64']).max()) for c in R.cases())


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: c['name'])
def test_spiral_generators_match_the_recorded_float64_run(golden, case):
    from poseprobe_amd import gen_videos
    c2w = R.invert(case['poses_w2c'])
    a = gen_videos.generate_spiral_path(c2w, case['bounds'], n_frames=R.N_SPIRAL)
    b = gen_videos.generate_spiral_path_dtu(c2w, n_frames=R.N_SPIRAL)
    assert a.dtype == np.float64 and a.shape == (R.N_SPIRAL, 3, 4) and b.shape == (R.N_SPIRAL, 3, 4)
    assert float(np.abs(a - golden[f'spiral.{case["name"]}']).max()) <= 1e-12
    assert float(np.abs(b - golden[f'spiral_dtu.{case["name"]}']).max()) <= 1e-12
    # a tensor comes back as a tensor, [n,3,4] float64 (the reference's contract)
    t = gen_videos.generate_spiral_path_dtu(torch.tensor(c2w), n_frames=R.N_SPIRAL, n_rots=1)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == (R.N_SPIRAL, 3, 4)
    # the frames are rigid poses looking at the scene: orthonormal, right-handed
    Rm = b[:, :, :3]
    assert float(np.abs(Rm.transpose(0, 2, 1) @ Rm - np.eye(3)).max()) < 1e-12 and np.all(np.linalg.det(Rm) > 0)


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: c['name'])
def test_oscillation_matches_the_recorded_run(golden, case):
    """float32 like the reference's pose algebra: allowed 4 x the float32 / float64 spread of the reference's own run."""
    from poseprobe_amd import camera, gen_videos
    w2c = torch.tensor(case['poses_w2c'], dtype=torch.float32)
    anchor = w2c[gen_videos.centre_most(w2c)]
    got = camera.get_novel_view_poses(None, anchor, N=R.N_PATH, scale=case['scale'])
    assert got.dtype == torch.float32 and tuple(got.shape) == (R.N_PATH, 3, 4)
    tol = 4 * _spread(golden, 'oscil')
    err = float(np.abs(got.numpy().astype(np.float64) - golden[f'oscil.{case["name"]}']).max())
    print(f'oscillation {case["name"]}: error {err:.3e}, tolerance {tol:.3e}')
    assert err <= tol


@pytest.mark.parametrize('case', R.cases(), ids=lambda c: c['name'])
def test_dtu_sequence_matches_the_recorded_run(golden, case):
    from poseprobe_amd import gen_videos
    w2c = torch.tensor(case['poses_w2c'], dtype=torch.float32)
    got = gen_videos.novel_view_poses(w2c, 'dtu', n_frames=R.N_PATH)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2 * R.N_PATH, 3, 4)
    tol = 4 * _spread(golden, 'dtu')
    err = float(np.abs(got.numpy().astype(np.float64) - golden[f'dtu.{case["name"]}']).max())
    print(f'dtu sequence {case["name"]}: error {err:.3e}, tolerance {tol:.3e}')
    assert err <= tol


def test_the_three_branches_of_novel_view_poses():
    from poseprobe_amd import camera, gen_videos
    case = R.cases()[1]
    w2c = torch.tensor(case['poses_w2c'], dtype=torch.float32)
    other = gen_videos.novel_view_poses(w2c, 'blender', n_frames=5)
    dtu = gen_videos.novel_view_poses(w2c, 'dtu', n_frames=5)
    llff = gen_videos.novel_view_poses(w2c, 'llff', n_frames=5, depth_range=tuple(case['bounds']))
    assert tuple(other.shape) == (5, 3, 4) and tuple(dtu.shape) == (10, 3, 4) and tuple(llff.shape) == (5, 3, 4)
    assert torch.equal(dtu[5:], other)
    want = camera.pose.invert(gen_videos.generate_spiral_path(camera.pose.invert(w2c), np.array(case['bounds']), n_frames=5))
    assert torch.equal(llff, want)
    with pytest.raises(ValueError):
        gen_videos.novel_view_poses(w2c, 'llff', n_frames=5)
