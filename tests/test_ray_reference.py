"""Grounds tests/ray_reference.py and tests/ray_cases.py without a GPU: the pose reference reproduces the pose fixture, the loss
references agree with the oracle's object_losses, and every crafted sampler input has, under the oracle alone, the properties
tests/test_hip_ray_kernels.py relies on."""
import numpy as np
import pytest
import torch

from oracle import native_ops
from oracle import voxurf_oracle as O
from tests import ray_cases as C
from tests import ray_reference as RR
from tests.helpers import assert_close, check, load, npf, scene_for

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------------- pose
def test_pose_chain_float32_reproduces_the_fixture():
    d = load('pose.npz')
    w2c, c2w, jac = RR.pose_chain(d['wu'], d['init'], None, torch.float32)
    assert w2c.dtype == c2w.dtype == jac.dtype == torch.float32 and jac.shape == (d['wu'].shape[0], 12, 6)
    assert_close(w2c, d['composed'], rtol=1e-6, atol=1e-6, name='w2c')
    assert_close(c2w, d['inverted'], rtol=1e-6, atol=1e-6, name='c2w')
    g = torch.einsum('vek,ve->vk', jac, torch.tensor(d['wsum']).reshape(-1, 12))
    assert_close(g, d['grad_wu'], rtol=1e-4, atol=1e-6, name='jac^T wsum')


@pytest.mark.parametrize('V', [1, 11, 50])
def test_pose_chain_float64_and_fixed_views(V):
    se3, init, mask = C.pose_case(V, masked=True)
    th = np.linalg.norm(se3[:, :3].astype(np.float64), axis=1)
    want = np.array([C.THETAS[v % 5] for v in range(V)])
    assert th.max() <= 3.0 and (th <= want).all() and th[0] == 0.0
    some = want > 0                                                # every magnitude of the cycle is there, in its own decade
    assert np.array_equal(np.round(np.log10(th[some])), np.round(np.log10(want[some])))
    assert V < 5 or len(set(np.round(np.log10(th[some])))) == 3 and (th[some] > 2.9).any()
    w2c, c2w, jac = RR.pose_chain(se3, init, mask, torch.float64)
    assert w2c.dtype == c2w.dtype == jac.dtype == torch.float64
    fixed = mask == 0
    assert fixed[0] and (V == 1 or (~fixed).any())
    assert np.array_equal(w2c.numpy()[fixed], init[fixed].astype(np.float64))
    assert (jac.numpy()[fixed] == 0).all()
    assert all((jac.numpy()[v] != 0).any() for v in np.nonzero(~fixed)[0])
    # the 12-pass Jacobian holds every view's own block: compare with the full Jacobian of one refined view
    if V > 1:
        v = int(np.nonzero(~fixed)[0][-1])
        s = torch.tensor(se3[v:v + 1], dtype=torch.float64)
        one = torch.autograd.functional.jacobian(
            lambda x: O.pose_invert(O.pose_compose_pair(O.se3_to_SE3(x), torch.tensor(init[v:v + 1], dtype=torch.float64))), s)
        assert np.array_equal(one.reshape(12, 6).numpy(), jac[v].numpy())


# ----------------------------------------------------------------------------------------------------------------------- losses
def test_clamp_bounds_are_the_fp32_programs():
    """torch clamps a float32 tensor at the float32 value of a Python bound: the gates of object_losses open exactly at the values
    the references (and the kernels) use."""
    for lo, hi, ref_lo, ref_hi in ((1e-6, 1 - 1e-6, RR.ENT_LO, RR.ENT_HI), (1e-3, 1.0 - 1e-3, RR.BCE_LO, RR.BCE_HI)):
        x = torch.tensor([0.0, 1.0])
        got = x.clamp(lo, hi).numpy()
        assert np.array_equal(got, np.array([ref_lo, ref_hi], F32))
        assert ref_hi == float(F32(1) - F32(ref_lo))


def test_loss_references_equal_the_oracle_losses():
    N, M, it, total = 257, 300, 1234, 10000
    ls, w_main, w_mask = 0.1, 1.0, 0.1
    r, s = C.ray_loss_case(N), C.sample_loss_case(M)
    leaf = lambda x: torch.tensor(x, requires_grad=True)
    out = dict(rgb_marched=leaf(r['rgbm']), alphainv_cum=leaf(r['alast']), cum_weights=leaf(r['cw'][:, None]),
               gradient=leaf(s['gradient']), grad_deform=leaf(s['grad_deform'].reshape(M, 3, 3)),
               sdf_correct=leaf(s['warp_out'][:, 3]), sdf_deform=leaf(s['sdf_deform']))
    S, Wt, loss = O.object_losses(out, torch.tensor(r['target']), torch.tensor(r['mask'][:, None]), it, total,
                                  weight_main=w_main, weight_tv_k0=0.0, weight_mask=w_mask)
    (loss * ls).backward()
    w_ent, w_def = Wt['weight_entropy_last'], Wt['grad_deform_constraint']
    assert Wt['grad_constraint'] == RR.W_EIKONAL and w_def == O.dynamic_weight(1e-1, 1e-3, it, total)
    ray = [RR.ray_losses(r['rgbm'], r['alast'], r['cw'], r['target'], r['mask'], w_main, w_ent, w_mask, ls, dtype=dt)
           for dt in (torch.float64, torch.float32)]
    smp = [RR.sample_losses(s['gradient'], s['grad_deform'], s['warp_out'], s['sdf_deform'], M, RR.W_EIKONAL, w_def, ls, dtype=dt)
           for dt in (torch.float64, torch.float32)]
    assert ray[1]['g_rgbm'].dtype == smp[1]['g_gradient'].dtype == torch.float32
    one = lambda x: npf(x).reshape(1)
    for key, name in (('mse', 'img_render'), ('entropy', 'weight_entropy_last'), ('bce', 'mask_render')):
        check(name, one(S[name]), one(ray[0][key]), one(ray[1][key]), one(ray[0][key]))
    for key, name in (('eikonal', 'grad_constraint'), ('grad_deform', 'grad_deform_constraint'),
                      ('correction', 'sdf_correct_constraint'), ('sdf_deform', 'sdf_deform_constraint')):
        check(name, one(S[name]), one(smp[0][key]), one(smp[1][key]), one(smp[0][key]))
    tot64, tot32 = (one(a['total']) + one(b['total']) for a, b in zip(ray, smp))
    check('loss', one(loss), tot64, tot32, tot64)
    for key, got in (('g_rgbm', out['rgb_marched'].grad), ('g_last', out['alphainv_cum'].grad), ('g_cw', out['cum_weights'].grad[:, 0])):
        check(key, got, ray[0][key], ray[1][key], np.abs(npf(ray[0][key])))
        assert np.array_equal(npf(got) == 0, npf(ray[0][key]) == 0), f'{key}: the gates differ'
    for key, got in (('g_gradient', out['gradient'].grad), ('g_grad_deform', out['grad_deform'].grad.reshape(M, 9)),
                     ('g_correction', out['sdf_correct'].grad), ('g_sdf_deform', out['sdf_deform'].grad)):
        check(key, got, smp[0][key], smp[1][key], np.abs(npf(smp[0][key])))
        assert np.array_equal(npf(got) == 0, npf(smp[0][key]) == 0), f'{key}: the zeros differ'
    # the seeded rows: gates shut outside the clamps and open at the bounds, zero subgradients at the kinks
    a, g_last = r['alast'], npf(ray[0]['g_last'])
    assert (g_last[(a < F32(RR.ENT_LO)) | (a > F32(RR.ENT_HI))] == 0).all() and (g_last[(a == F32(RR.ENT_LO)) | (a == F32(RR.ENT_HI))] != 0).all()
    assert ((a == F32(RR.ENT_LO)).sum(), (a == F32(RR.ENT_HI)).sum(), (a == 0).sum(), (a == 1).sum()) == (2, 2, 2, 2)
    c, g_cw = r['cw'], npf(ray[0]['g_cw'])
    assert (g_cw[(c < F32(RR.BCE_LO)) | (c > F32(RR.BCE_HI))] == 0).all() and (g_cw[(c == F32(RR.BCE_LO)) | (c == F32(RR.BCE_HI))] != 0).all()
    assert ((c == F32(RR.BCE_LO)).sum(), (c == F32(RR.BCE_HI)).sum()) == (2, 2)
    gg = npf(smp[0]['g_gradient'])
    assert (gg[[0, 1, M - 5, M - 4]] == 0).all() and (npf(smp[0]['g_grad_deform'])[[2, M - 3], 3:6] == 0).all()
    assert (npf(smp[0]['g_correction'])[[3, M - 2]] == 0).all() and (npf(smp[0]['g_sdf_deform'])[[4, M - 1]] == 0).all()


def test_batch_norm_variant_rescales_the_normalised_terms():
    """batch_norm = (sum(mask), M) is the plain case; other values rescale the MSE and the sample terms, not entropy and BCE."""
    N, M = 255, 256
    r, s = C.ray_loss_case(N), C.sample_loss_case(M)
    args = (r['rgbm'], r['alast'], r['cw'], r['target'], r['mask'], 1.0, 0.01, 0.1, 0.5)
    sargs = (s['gradient'], s['grad_deform'], s['warp_out'], s['sdf_deform'], M, 1.0, 0.05, 0.5)
    plain, splain = RR.ray_losses(*args), RR.sample_losses(*sargs)
    same = RR.ray_losses(*args, batch_norm=(float(r['mask'].sum()), float(M)))
    assert all(np.array_equal(npf(plain[k]), npf(same[k])) for k in plain)
    bn = (2.0 * float(r['mask'].sum()), 4.0 * M)
    b, sb = RR.ray_losses(*args, batch_norm=bn), RR.sample_losses(*sargs, batch_norm=bn)
    assert float(b['mse']) == float(plain['mse']) / 2 and np.array_equal(npf(b['g_rgbm']), npf(plain['g_rgbm']) / 2)
    assert float(b['entropy']) == float(plain['entropy']) and np.array_equal(npf(b['g_cw']), npf(plain['g_cw']))
    for k in ('eikonal', 'grad_deform', 'correction', 'sdf_deform', 'g_gradient', 'g_grad_deform', 'g_correction', 'g_sdf_deform'):
        assert np.array_equal(npf(sb[k]), npf(splain[k]) / 4), k


def test_sample_losses_count_handling():
    s = C.sample_loss_case(257)
    args = (s['gradient'], s['grad_deform'], s['warp_out'], s['sdf_deform'])
    over, full = RR.sample_losses(*args, 257 + 5, 1.0, 0.05, 1.0), RR.sample_losses(*args, 257, 1.0, 0.05, 1.0)
    assert over['M'] == full['M'] == 257 and float(over['total']) == float(full['total'])
    empty = RR.sample_losses(*args, 0, 1.0, 0.05, 1.0)
    assert empty['M'] == 0 and float(empty['total']) == 0 and empty['g_gradient'].shape == (0, 3)
    assert RR.sample_losses(*args, 256, 1.0, 0.05, 1.0)['g_sdf_deform'].shape == (256,)


# --------------------------------------------------------------------------------------------------------------------- samplers
@pytest.mark.parametrize('G,n_rays,kind', C.SAMPLER_CASES)
def test_crafted_sampler_inputs_have_their_properties_under_the_oracle(G, n_rays, kind):
    scene = scene_for(G, stepsize=0.5)
    S = scene.n_samples()
    assert S == {24: 87, 40: 143}[G]
    o, d, jit = C.sampler_rays(n_rays, kind)
    assert o.dtype == d.dtype == jit.dtype == F32 and (0 <= jit).all() and (jit < 1).all()
    to, td = torch.tensor(o), torch.tensor(d)
    chunks = (S + 63) // 64
    counts = []
    for j in (torch.tensor(jit), None):
        _, mask_out, _, _, _ = O.sample_dense(scene, to, td, j)
        counts.append((~mask_out).sum(1).numpy())
    n_steps = native_ops.sample_pts_on_rays(to, td, scene.xyz_min, scene.xyz_max, scene.near, 1e9,
                                            float(scene.stepsize * scene.voxel_size))[4].numpy()
    _, ray_id, _, _, _ = O.sample_variable(scene, to, td)
    counts.append(np.bincount(ray_id.numpy(), minlength=n_rays))
    for cnt in counts:
        if kind == 'miss':
            assert cnt.sum() == 0
            continue
        assert cnt.sum() > 0
        assert cnt.max() > 64 * (chunks - 1), 'no ray carries its offset into the last 64-lane chunk'
        if n_rays >= 4:
            assert (cnt == 0).any()
        if n_rays > 1024:
            assert cnt[1024:].sum() > 0 and cnt[:1024].sum() > 0, 'the scan carries nothing across its pass boundary'
    if kind == 'mixed':
        assert n_steps.max() > 64 * (chunks - 1)
        m = min(n_rays, C.N_SPECIAL)
        mn, mx = scene.xyz_min.numpy(), scene.xyz_max.numpy()
        zeros = (d[:m] == 0).sum(1)
        assert zeros.tolist() == [0, 1, 2, 0, 0, 0, 0, 0][:m]
        for cnt in counts:
            assert cnt[0] > 64 * (chunks - 1)
            assert all(cnt[k] == 0 for k in (3, 5) if k < m) and all(cnt[k] > 0 for k in (1, 2, 4, 6, 7) if k < m)
        if m > 4:
            assert ((mn < o[4]) & (o[4] < mx)).all()
        if m > 5:
            assert ((o[5] - C.CENTRE) @ d[5]) > 0
        if m > 7:
            assert jit[6] == 0 and jit[7] == np.nextafter(F32(1), F32(0))
        if n_rays >= 1023:
            assert (d[n_rays - C.N_SPECIAL:] == 0).sum(1).max() == 2
