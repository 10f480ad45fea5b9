"""CPU checks of the two other branches of Voxurf.forward / Voxurf.inference (use_deform=False, fast_color_thres > 0):
the float64-capable restatement the kernel tests are measured against IS the reference's function (compared with a recorded run
of the reference, tests/golden/forward_variants_g24.npz), the returned dict has the reference's keys per mode, and what is still
out of scope refuses with a message that says so."""
import numpy as np
import pytest
import torch

from tests import forward_variants_reference as R
from tests.helpers import assert_close, load, scene_for


@pytest.fixture(scope='module')
def golden():
    return load('forward_variants_g24.npz')


def test_the_fixture_meets_the_conditions_the_exact_index_checks_rest_on(golden):
    d = golden
    N, thres = int(d['n_rand']), float(d['thres'])
    M = d['samples.ray_id'].shape[0]
    assert N == 192 and M % 64 != 0 and M % 4096 != 0
    n = np.bincount(d['samples.ray_id'], minlength=N)
    assert (n == 0).any(), 'a ray that misses the box'
    for first, case in (('plain', 'plain_thres'),):           # the threshold-free run of the same branch holds the first composite
        w = d[f'{first}.out.weights']
        assert R.margin_to_threshold(w, thres) > 1e-3
        k = np.bincount(d['samples.ray_id'][d[f'{case}.kept']], minlength=N)
        assert ((k == 0) & (n > 0)).any() and ((k == n) & (n > 0)).any()
    for case in ('thres', 'plain_thres'):
        assert d[f'{case}.out.mask'].sum() == d[f'{case}.kept'].shape[0] == d[f'{case}.out.weights'].shape[0] > 0
        assert np.array_equal(np.nonzero(d[f'{case}.out.mask'])[0], d[f'{case}.kept'])


def test_restatement_is_the_reference_function(golden):
    """plain_geometry on the reference sampler's points gives the reference's raw_alpha / gradient (same torch operators: a few
    float32 roundings apart), the mask of its weights is the recorded kept set, and the second composite of the kept alphas gives
    the recorded weights."""
    from oracle import voxurf_oracle as O
    d = golden
    P = R.fixture_params(d)
    scene = scene_for(int(d['G']))
    t = torch.tensor
    gs = int(d['global_step'])
    pts, ray_id = t(d['samples.pts']), t(d['samples.ray_id']).long()
    dirs = t(d['viewdirs'])[ray_id]
    dist = scene.stepsize * scene.voxel_size
    inv_s = torch.ones(1) / (torch.ones(1) * O.s_val_at(scene, gs))
    sdf_final, gradient, alpha = R.plain_geometry(t(P['P.sdf'])[0, 0], t(P['P.sdf_alpha']), t(P['P.sdf_beta']), pts, dirs,
                                                  scene.xyz_min, scene.xyz_max, scene.voxel_size, dist, inv_s)
    assert_close(gradient, d['plain.out.gradient'], rtol=1e-5, atol=1e-6, name='gradient')
    assert_close(alpha, d['plain.out.raw_alpha'], rtol=1e-5, atol=1e-7, name='raw_alpha')
    N, thres = int(d['n_rand']), float(d['thres'])
    w, last = O.Alphas2Weights.apply(alpha, ray_id, N)
    assert_close(w, d['plain.out.weights'], rtol=1e-5, atol=1e-8, name='first composite')
    kept = torch.nonzero(R.threshold_mask(w, thres))[:, 0]
    assert np.array_equal(kept.numpy(), d['plain_thres.kept'])
    assert_close(alpha[kept], d['plain_thres.out.raw_alpha'], rtol=1e-5, atol=1e-7, name='kept alpha')
    assert_close(gradient[kept], d['plain_thres.out.gradient'], rtol=1e-5, atol=1e-6, name='kept gradient')
    w2, last2 = O.Alphas2Weights.apply(alpha[kept], ray_id[kept], N)
    assert_close(w2, d['plain_thres.out.weights'], rtol=1e-5, atol=1e-8, name='second composite')
    assert_close(last2, d['plain_thres.out.alphainv_cum'], rtol=1e-5, atol=1e-7, name='alphainv_cum')
    # the deformation outputs of a thresholded run keep every sample's row (voxurf_coarse.py:1086-1091)
    assert d['thres.out.sdf_deform'].shape[0] == d['thres.out.grad_deform'].shape[0] == d['thres.out.sdf_correct'].shape[0] == pts.shape[0]
    assert d['thres.out.gradient'].shape[0] == d['thres.kept'].shape[0] < pts.shape[0]


def test_float32_restatement_stays_within_rounding_of_its_float64_self():
    """The yardstick of the kernel tests: on their own inputs the float32 run of the restatement is a few float32 ulps from the
    float64 run wherever both read the same cell."""
    for shape, seed in (((8, 8, 8), 1), ((6, 8, 10), 2)):
        case = R.kernel_case(shape, seed)
        r64, r32 = R.kernel_case_reference(case, torch.float64), R.kernel_case_reference(case, torch.float32)
        assert case['lattice'].sum() >= 8 and (~case['lattice']).sum() >= 40
        for k in ('sdf_final', 'gradient', 'alpha'):
            assert np.abs(r32[k] - r64[k]).max() <= 64 * R.ulp32(np.abs(r64[k]).max()), k


def test_returned_dict_keys_per_mode(golden):
    from poseprobe_amd import voxurf_coarse as Model
    for case in R.CASES:
        deform, _ = R.CASE_SWITCHES[case]
        want = set(Model.FORWARD_KEYS) | (set(Model.FORWARD_DEFORM_KEYS) if deform else set())
        assert set(golden[f'{case}.keys'].tolist()) == want, case


def _model(**kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd import voxurf_coarse as Model
    rs = syn.range_shape()
    args = dict(num_voxels=8 ** 3, num_voxels_base=8 ** 3, alpha_init=1e-2, rgbnet_dim=12, rgbnet_direct=True, rgbnet_depth=4,
                rgbnet_width=128, posbase_pe=5, viewbase_pe=1, geo_rgb_dim=3, s_ratio=50, s_start=0.2, barf_c2f=[0.6, 1],
                i_train=np.arange(3), N_iters=10000, HW=np.array([[8, 8]] * 3), range_shape=rs, rect_size=rs.tolist(), camera_noise=0.)
    args.update(kw)
    return Model.Voxurf(syn.XYZ_MIN, syn.XYZ_MAX, **args)


def test_remaining_refusals_say_what_is_out_of_scope():
    from poseprobe_amd.engine import RenderCore, SceneConfig
    from poseprobe_amd import synthetic as syn
    for kw in (dict(smooth_ksize=3), dict(s_learn=True), dict(rgbnet_width=64), dict(rgbnet_depth=3)):
        with pytest.raises(NotImplementedError, match='shipped e2e configuration'):
            _model(**kw)
    rays = torch.zeros(4, 3)
    for mode in ('raw', 'grad_conv'):
        m = _model(grad_mode=mode)
        with pytest.raises(NotImplementedError, match=f"use_deform=False with grad_mode='{mode}'"):
            m(rays, rays, rays, use_deform=False, global_step=1, **R.RENDER_KWARGS)
        with pytest.raises(NotImplementedError, match='grad_mode'):
            m.query_sdf_point_wocuda_render(rays, rays + 1, use_deform=False, **R.RENDER_KWARGS)
    m = _model(fast_color_thres=1e-3)
    with pytest.raises(NotImplementedError, match='k0_grad_tv'):
        m.k0_total_variation(k0_grad_tv=1.0)
    # both switches are accepted now: what stops a CPU call is the device check, not a refusal of the branch
    for deform in (True, False):
        with pytest.raises(RuntimeError, match='HIP path only'):
            m(rays, rays, rays, use_deform=deform, global_step=1, **R.RENDER_KWARGS)
    # the fused train step keeps the default branch: the core refuses the combination before it touches a buffer
    core = RenderCore(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, 8 ** 3))
    for kw in (dict(side_by_side=True), dict(composite=False), dict(before_k0_use=lambda: None)):
        for variant in (dict(use_deform=False), dict(color_thres=1e-3)):
            with pytest.raises(ValueError, match='not inside the fused train step'):
                core.forward(None, None, None, None, None, None, 1.0, None, **kw, **variant)
    for kw in (dict(priors=(0, 0, 0, None, None)), dict(march_done=True)):
        with pytest.raises(ValueError, match='not inside the fused train step'):
            core.backward(None, None, None, None, None, None, 1.0, None, None, None, None, None, use_deform=False, **kw)
