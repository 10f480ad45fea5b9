"""Pins the float64 stage references (tests/stage_reference.py) to the reference model: composed in float32 on the inputs of
forward_g8_s10.npz they reproduce the fixture's out.* values at the tolerances of test_analytic_derivation.py, and in float64
they stay float64 throughout (no float32 constant silently demotes them)."""
import numpy as np
import torch

from oracle import voxurf_oracle as O
from tests import stage_reference as SR
from tests.helpers import assert_close, load, params_from_npz, scene_for


def _warp_out(P, scene, pts):
    """[M,16] warp outputs with the Jacobian rows the kernels take: wo[4 + 4i + j] = d out_j / d p_i (minus delta_ij for j < 3)."""
    x = pts.detach().clone().requires_grad_(True)
    deform, corr = O.warp_mlp(P, scene, x)
    out = torch.cat([deform, corr], -1)
    J = torch.stack([torch.autograd.grad(out[:, c].sum(), x, retain_graph=True)[0] for c in range(4)], -1)  # [M, i, c]
    return torch.cat([out, J.reshape(-1, 12)], -1).detach()


def _compose(d, dtype):
    scene = scene_for(d['G'])
    P = params_from_npz(d)
    gs = int(d['global_step'])
    ro, rd, vd = (torch.tensor(d[k]) for k in ('rays_o', 'rays_d', 'viewdirs'))
    pts, mask_out, step, _, _ = O.sample_dense(scene, ro, rd, torch.tensor(d['jitter']))
    ray_pts, ray_id, _, _ = O.compact_samples(pts, mask_out, step)
    wo = _warp_out(P, scene, ray_pts)
    s_t = torch.ones(1) * O.s_val_at(scene, gs)
    inv_s = float((torch.ones(1) / s_t)[0])
    dist = float(scene.stepsize * scene.voxel_size)
    sdf_ab = torch.cat([P['sdf_alpha'], P['sdf_beta']])
    geo = SR.geometry(ray_pts, wo, vd, ray_id, P['sdf'][0, 0], sdf_ab, inv_s, dist, scene.xyz_min, scene.xyz_max, dtype=dtype,
                      g_alpha=torch.ones(len(ray_pts)))
    progress = gs / scene.N_iters
    pe_w = torch.cat([O.barf_weights(scene, progress, scene.posbase_pe), O.barf_weights(scene, progress, scene.viewbase_pe)])
    col = SR.color_feat(P['k0'][0], ray_pts, vd, ray_id, geo['gradient'], pe_w, scene.posbase_pe, scene.viewbase_pe,
                        scene.xyz_min, scene.xyz_max, dtype=dtype)
    width = scene.k0_dim + 3 + 6 * scene.posbase_pe + 3 + 6 * scene.viewbase_pe + 3
    Pd = {'rgbnet': [(w.to(dtype), b.to(dtype)) for w, b in P['rgbnet']]}
    rgb = torch.sigmoid(O.rgbnet_mlp(Pd, col['feat'][:, :width]))
    rs = np.concatenate([[0], np.cumsum(np.bincount(ray_id.numpy(), minlength=len(ro)))])
    mar = SR.march(geo['alpha'].float(), rgb, rs, scene.bg, dtype=dtype)
    return geo, col, rgb, mar


def test_composed_float32_stages_reproduce_the_reference_forward():
    d = load('forward_g8_s10.npz')
    geo, col, rgb, mar = _compose(d, torch.float32)
    tol = dict(rtol=1e-4, atol=2e-6, scaled=1e-6)
    assert_close(geo['alpha'], d['out.raw_alpha'], name='raw_alpha', **tol)
    assert_close(geo['gradient'], d['out.gradient'], name='gradient', **tol)
    assert_close(geo['grad_deform'].reshape(-1, 3, 3), d['out.grad_deform'], name='grad_deform', **tol)
    assert_close(geo['sdf_deform'], d['out.sdf_deform'], name='sdf_deform', **tol)
    assert_close(rgb, d['out.raw_rgb'], name='raw_rgb', **tol)
    assert_close(mar['weights'], d['out.weights'], name='weights', **tol)
    assert_close(mar['alphainv_last'], d['out.alphainv_cum'], name='alphainv_cum', **tol)
    assert_close(mar['cum_weights'][:, None], d['out.cum_weights'], name='cum_weights', **tol)
    assert_close(mar['rgb_marched'], d['out.rgb_marched'], name='rgb_marched', **tol)


def test_float64_references_stay_float64_and_agree_with_float32():
    d = load('forward_g8_s10.npz')
    geo64, col64, rgb64, mar64 = _compose(d, torch.float64)
    geo32, col32, rgb32, mar32 = _compose(d, torch.float32)
    for name, x in (('alpha', geo64['alpha']), ('gradient', geo64['gradient']), ('pts_grad', geo64['pts_grad']),
                    ('warp_out_grad', geo64['warp_out_grad']), ('sdf_ab', geo64['sdf_ab']), ('feat', col64['feat']),
                    ('rgb', rgb64), ('weights', mar64['weights'])):
        assert x.dtype == torch.float64, name
    assert_close(geo32['pts_grad'], geo64['pts_grad'], rtol=1e-3, atol=1e-6, scaled=1e-5, name='pts_grad')
    assert_close(geo32['warp_out_grad'], geo64['warp_out_grad'], rtol=1e-3, atol=1e-6, scaled=1e-5, name='warp_out_grad')
    assert_close(rgb32, rgb64, rtol=1e-5, atol=1e-6, name='rgb')
    # the fixture takes the cos < 0 branch of the viewdir gate, and the unclipped alpha never exceeds 1
    assert (geo64['cos'] < 0).any() and (geo64['a_un'] <= 1).all()


def test_march_reference_backward_is_the_native_scan_gradient():
    """Gradient of the float64 weights equals the .cu backward (oracle.native_ops) evaluated on the same inputs, to fp32
    accuracy: the reference's weights really are the functions of alpha the scan defines up to i_end."""
    from oracle import native_ops
    rng = np.random.RandomState(0)
    lens = np.array([0, 1, 5, 70, 200])
    rs = np.concatenate([[0], np.cumsum(lens)])
    M, N = int(rs[-1]), len(lens)
    alpha = rng.uniform(0, 0.08, M).astype(np.float32)
    gw, gl = rng.randn(M).astype(np.float32), rng.randn(N).astype(np.float32)
    ref = SR.march(alpha, np.zeros((M, 3), np.float32), rs, 0.0, g_w=gw, g_last=gl)
    ray_id = torch.repeat_interleave(torch.arange(N), torch.tensor(lens))
    w, T, last, i_s, i_e = native_ops.alpha2weight(torch.tensor(alpha), ray_id, N)
    g = native_ops.alpha2weight_backward(torch.tensor(alpha), w, T, last, i_s, i_e, N, torch.tensor(gw), torch.tensor(gl))
    assert_close(g, ref['g_alpha'], rtol=1e-4, atol=1e-6, scaled=1e-6, name='g_alpha')
