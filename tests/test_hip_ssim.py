"""GPU tests of the SSIM kernel (csrc/pp_ssim.hip) and of the scores built on it (poseprobe_amd.evaluation)
against the recorded float64 run of the reference's rgb_ssim (tests/golden/eval_metrics.npz).

Accuracy bound of a case, for the value and for the map's maximum separately: 4 x the error of the reference's own function fed
the case's arrays rounded to float32 (recorded beside the float64 run), but at least FLOOR_ULPS float32 ulps of the value (of 1
for the map): the kernel's results are float32, so half an ulp is lost to their rounding in every case, also where the
yardstick is 0 (identical images, all zeros against all ones) or, for the value, averages its errors away."""
import types

import numpy as np
import pytest
import torch

from tests import evaluation_reference as R
from tests.helpers import load

pytestmark = pytest.mark.gpu

FLOOR_ULPS = 4


@pytest.fixture(scope='module')
def golden():
    return load('eval_metrics.npz')


@pytest.fixture(scope='module')
def cases(golden):
    from poseprobe_amd import ops
    T = ops.ssim_tile()
    assert T == int(golden['tile']), 'tests/golden/eval_metrics.npz was recorded for another tile edge: rerun tools/make_eval_golden.py'
    return R.ssim_cases(T)


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def test_ssim_matches_the_recorded_reference_in_every_case(golden, cases):
    from poseprobe_amd import evaluation as E
    for case in cases:
        kw = dict(max_val=case['max_val'], filter_size=case['fs'])
        x = torch.tensor(np.stack([p[0] for p in case['pairs']]), dtype=torch.float32).cuda()
        y = torch.tensor(np.stack([p[1] for p in case['pairs']]), dtype=torch.float32).cuda()
        values, maps = E.rgb_ssim(x, y, **kw), E.rgb_ssim(x, y, return_map=True, **kw)
        assert values.shape == (len(case['pairs']),) and values.dtype == torch.float32 and values.is_cuda
        for i in range(len(case['pairs'])):
            key = f'ssim.{case["name"]}.{i}'
            ref_v, ref_m = float(golden[key + '.value']), golden[key + '.map']
            bound_v = max(4 * abs(float(golden[key + '.value32']) - ref_v), FLOOR_ULPS * _ulp32(ref_v))
            bound_m = max(4 * float(np.abs(golden[key + '.map32'] - ref_m).max()), FLOOR_ULPS * _ulp32(1.0))
            err_v = abs(float(values[i]) - ref_v)
            got_m = maps[i].cpu().numpy().astype(np.float64)
            assert got_m.shape == ref_m.shape, key
            err_m = float(np.abs(got_m - ref_m).max())
            print(f'{key}: value {float(values[i]):.9g} off by {err_v:.3e} (bound {bound_v:.3e}), map off by {err_m:.3e} (bound {bound_m:.3e})')
            assert err_v <= bound_v, (key, err_v, bound_v)
            assert err_m <= bound_m, (key, err_m, bound_m)
            # a single view [H,W,3] gives the same bits, 0-dim; so does a view of the batch alone
            single = E.rgb_ssim(x[i], y[i], **kw)
            assert single.shape == () and torch.equal(_bits(single), _bits(values[i])), key
            # the mean of the returned map is the value, to float32 rounding (the map's own rounding averaged over its pixels)
            assert abs(float(maps[i].double().mean()) - float(values[i])) <= 1.5 * _ulp32(ref_v), key
    assert abs(float(E.rgb_ssim(*(torch.tensor(a, dtype=torch.float32).cuda() for a in cases[6]['pairs'][0]), 1.)) - 1) <= 1e-6
    assert cases[6]['name'] == 'identical'


def test_ssim_is_bit_reproducible_and_independent_of_the_batch(cases):
    from poseprobe_amd import evaluation as E
    case = cases[-1]
    assert case['name'] == 'batch3' and len(case['pairs']) == 3
    x = torch.tensor(np.stack([p[0] for p in case['pairs']]), dtype=torch.float32).cuda()
    y = torch.tensor(np.stack([p[1] for p in case['pairs']]), dtype=torch.float32).cuda()
    a, b = E.rgb_ssim(x, y, 1.), E.rgb_ssim(x, y, 1.)
    assert torch.equal(_bits(a), _bits(b))
    m1, m2 = E.rgb_ssim(x, y, 1., return_map=True), E.rgb_ssim(x, y, 1., return_map=True)
    assert torch.equal(_bits(m1), _bits(m2))
    for i in range(3):
        alone = E.rgb_ssim(x[i:i + 1], y[i:i + 1], 1.)
        assert torch.equal(_bits(alone[0]), _bits(a[i]))
        assert torch.equal(_bits(E.rgb_ssim(x[i], y[i], 1., return_map=True)), _bits(m1[i]))
    # the value does not depend on whether the map is written (ops level: one call with the map, one without)
    from poseprobe_amd import ops
    V, H, W, C = x.shape
    work = torch.empty(ops.ssim_workspace(V, H, W, 11), dtype=torch.uint8, device='cuda')
    v0, v1 = torch.empty(V, device='cuda'), torch.empty(V, device='cuda')
    smap = torch.empty(V, H - 10, W - 10, C, device='cuda')
    ops.ssim(x, y, 1., 11, 1.5, 0.01, 0.03, work, v0)
    ops.ssim(x, y, 1., 11, 1.5, 0.01, 0.03, work, v1, smap)
    assert torch.equal(_bits(v0), _bits(v1)) and torch.equal(_bits(v0), _bits(a)) and torch.equal(_bits(smap), _bits(m1))
    # arrays are uploaded; 1, 2 and 4 channels run (the fourth channel of a batch equals the single-channel call on it)
    rs = np.random.RandomState(5)
    p, q = rs.rand(40, 37, 4).astype(np.float32), rs.rand(40, 37, 4).astype(np.float32)
    m4 = E.rgb_ssim(p, q, 1., return_map=True)
    for c in range(4):
        m1c = E.rgb_ssim(np.ascontiguousarray(p[..., c:c + 1]), np.ascontiguousarray(q[..., c:c + 1]), 1., return_map=True)
        assert torch.equal(_bits(m1c[..., 0]), _bits(m4[..., c]))
    ref = R.rgb_ssim(p[..., :3].astype(np.float64), q[..., :3].astype(np.float64), 1., return_map=True)
    assert np.abs(m4[..., :3].cpu().numpy() - ref).max() <= FLOOR_ULPS * _ulp32(1.0)


def test_image_metrics_psnrs_equal_psnr_terms():
    from poseprobe_amd import evaluation as E
    from poseprobe_amd import nvs_fun
    rs = np.random.RandomState(3)
    rgb, gt = rs.rand(2, 24, 31, 3).astype(np.float32), rs.rand(2, 24, 31, 3).astype(np.float32)
    mask = (rs.rand(2, 24, 31, 1) < 0.5).astype(np.float32)
    m = E.image_metrics(rgb, gt, mask)
    assert all(m[k].shape == (2,) and m[k].is_cuda and m[k].dtype == torch.float32 for k in ('psnr', 'psnr_fore', 'psnr_back', 'ssim'))
    # psnr_terms sums float32 in numpy (pairwise: relative error below 1e-6); 10 / ln 10 x that is below 1e-5 dB
    for i in range(2):
        want = nvs_fun.psnr_terms(rgb[i], gt[i], mask[i])
        got = [float(m[k][i]) for k in ('psnr', 'psnr_fore', 'psnr_back')]
        assert np.abs(np.array(got) - np.array(want, np.float64)).max() <= 1e-5, (got, want)
        assert float(m['ssim'][i]) == float(E.rgb_ssim(rgb[i], gt[i], 1.))
    one = E.image_metrics(rgb[0], gt[0])
    assert one['psnr'].shape == () and float(one['psnr_fore']) == 0. and float(one['psnr_back']) == 0.
    assert abs(float(one['psnr']) - nvs_fun.psnr_terms(rgb[0], gt[0])[0]) <= 1e-5


def test_evaluate_viewpoints_scores_the_views_render_viewpoints_renders():
    from poseprobe_amd import evaluation as E
    from poseprobe_amd import nvs_fun
    from tests.test_hip_dropin import make_model
    d = load('viewpoints_g24.npz')
    m = make_model(d)
    H, W = int(d['H']), int(d['W'])
    rk = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, inverse_y=True, flip_x=False, flip_y=False)
    cfg = types.SimpleNamespace(data=types.SimpleNamespace(flip_x=False, flip_y=False))
    nv = d['w2c'].shape[0]
    args = (m, torch.tensor(d['w2c']), cfg, np.array([[H, W]] * nv), d['Ks'], False, rk)
    rgbs, _ = nvs_fun.render_viewpoints(*args, gt_imgs=d['gt'], masks=d['masks'])
    last = nvs_fun.render_viewpoints.last
    r = E.evaluate_viewpoints(*args, d['gt'], masks=d['masks'])
    assert len(r['rgbs']) == nv and all(t.is_cuda for t in r['rgbs'])
    for i in range(nv):
        assert np.array_equal(r['rgbs'][i].cpu().numpy(), rgbs[i])                    # the same kernels on the same rays
    for k in ('psnr', 'psnr_fore', 'psnr_back'):
        assert np.abs(np.array(r['per_view'][k]) - np.array(last['per_view'][k])).max() <= 1e-5, k
        assert abs(r[k] - last[k]) <= 1e-5
    want = E.rgb_ssim(rgbs, d['gt'], 1.).cpu().numpy()
    assert np.array_equal(np.array(r['per_view']['ssim'], np.float32), want)
    assert abs(r['ssim'] - float(want.mean())) <= 1e-7
    assert np.abs(want - [R.rgb_ssim(rgbs[i].astype(np.float64), d['gt'][i].astype(np.float64), 1.) for i in range(nv)]).max() <= 4 * _ulp32(1.)


def test_trainer_pose_error_is_evaluate_poses_of_the_engines_poses():
    from poseprobe_amd import bg_nerf
    from poseprobe_amd import evaluation as E
    from poseprobe_amd.trainer import DualBranchTrainer
    from tests.test_hip_step import build_engine
    d = load('forward_g24_s10.npz')
    eng, _ = build_engine(d)
    eng.zero_grads()
    opt = bg_nerf.default_options(sample_intvs=16)
    opt.nerf.rand_rays = 96
    torch.manual_seed(2)
    tr = DualBranchTrainer(eng, opt, max_iter=20, incremental_step=4)            # two active views until step 4
    for step in range(2):
        tr.train_step(step)
    assert tr.n_active == 2
    GT = torch.tensor(R.ground_truth_poses(3), dtype=torch.float32).cuda()
    se3 = eng.se3.clone()
    error, aligned, sim3 = tr.pose_error(GT)
    assert torch.equal(eng.se3, se3) and error.R.shape == (2,) and error.t.shape == (2,) and aligned.shape == (2, 3, 4)
    want, want_aligned, _ = E.evaluate_poses(eng.w2c[:2], GT[:2])
    assert torch.equal(error.R, want.R) and torch.equal(error.t, want.t) and torch.equal(aligned, want_aligned)
    assert sim3.type == 'traj_align' and bool(torch.isfinite(error.R).all()) and bool(torch.isfinite(error.t).all())
