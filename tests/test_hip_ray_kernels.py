"""The first kernels of an object-branch step, one at a time, on seeded inputs with the edge cases planted (tests/ray_cases.py):
pose exponential with its Jacobian, ray generation, the dense and the variable-length sampler, the two loss kernels.

Three kinds of assertion, and no other tolerance:
  * against a float64 reference (tests/ray_reference.py): the rule of tests/test_hip_stage_kernels.py (helpers.check),
    |hip - ref64| <= 2 |ref32 - ref64| + 8 eps32 * scale, scale = the largest term of the sum behind the entry;
  * bit-exact promises (rays, both samplers, rows a kernel must not touch, closed clamp gates): np.array_equal against
    the fp32 oracle;
  * integers: exact.
Every output buffer has guard rows filled with a sentinel that must come back unchanged.

pp_sample_dense / pp_sample_var stage the per-ray counts in the first n_rays entries of `ray_id` (pp_rays.hip; hence their
requirement capacity >= n_rays): where count < n_rays (a batch that misses the box) those entries hold counts, not the sentinel; everything from
max(count, n_rays) on is untouched.
"""
import numpy as np
import pytest
import torch

from oracle import native_ops
from oracle import voxurf_oracle as O
from tests import ray_cases as C
from tests import ray_reference as RR
from tests.helpers import check, cu, npf, scene_for

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT, ISENT, GUARD = 1234.5, -7, 8
DTYPES = (torch.float64, torch.float32)


def full(rows, *shape, value=SENT, dtype=torch.float32):
    return torch.full((rows,) + shape, value, dtype=dtype, device='cuda')


def ifull(rows, *shape):
    return full(rows, *shape, value=ISENT, dtype=torch.int32)


def host(t):
    return t.detach().cpu().numpy()


def untouched(name, t, start, value=None):
    rest = host(t)[start:]
    assert (rest == (value if value is not None else (ISENT if t.dtype == torch.int32 else SENT))).all(), \
        f'{name}: rows from {start} on were written'


def _cfg(G, **kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig
    return SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, int(G) ** 3, out_range=float(syn.range_shape().max()), **kw)


# ------------------------------------------------------------------------------------------------------------------------- pose
def seq_sum32(jac, g):
    """sum_e jac[v,e,k] * g[v,e] in float32, e ascending: a plain fp32 evaluation of jac^T g."""
    jac, g = np.asarray(jac, F32), np.asarray(g, F32)
    s = np.zeros((jac.shape[0], 6), F32)
    for e in range(12):
        s = s + jac[:, e, :] * g[:, e, None]
    return s


@pytest.mark.parametrize('masked', [False, True], ids=['all', 'mask'])
@pytest.mark.parametrize('V', [1, 11, 50])
def test_pose_fwd_jacobian_and_bwd(V, masked):
    """w2c, c2w and the whole Jacobian against the float64 pose chain; V = 11: a view's six tangent threads straddle two 64-thread
    work-groups.  The scale of a view is the largest term of its series and products (ray_reference.pose_term_scale)."""
    from poseprobe_amd import ops
    se3, init, mask = C.pose_case(V, masked)
    r64, r32 = (RR.pose_chain(se3, init, mask, dt) for dt in DTYPES)
    w2c, c2w, jac = full(V + GUARD, 3, 4), full(V + GUARD, 3, 4), full(V + GUARD, 12, 6)
    ops.pose_fwd(cu(se3), cu(init), None if mask is None else cu(mask, torch.int32), w2c, c2w, jac)
    scale = RR.pose_term_scale(se3, init)[:, None, None]
    for name, got, k in (('w2c', w2c, 0), ('c2w', c2w, 1), ('jac', jac, 2)):
        untouched(name, got, V)
        check(name, got[:V], r64[k], r32[k], scale)
    if masked:
        fixed = mask == 0
        assert fixed[0] and np.array_equal(host(w2c)[:V][fixed], init[fixed]), 'a fixed view must return w2c_init bit for bit'
        assert (host(jac)[:V][fixed] == 0).all()
    # backward: se3_grad = jac^T c2w_grad
    g = np.random.RandomState(V).normal(size=(V, 12)).astype(F32)
    grad = full(V + GUARD, 6)
    ops.pose_bwd(jac[:V], cu(g), grad[:V])
    untouched('se3_grad', grad, V)
    terms = npf(r64[2]) * g[:, :, None]
    # (1) against the float64 Jacobian: an entry of jac is itself a sum with terms up to the view's scale
    check('se3_grad', grad[:V], terms.sum(1), seq_sum32(host(r32[2]), g), scale[:, 0] * np.abs(g).max(1, keepdims=True))
    # (2) against the float64 product of the kernel's own Jacobian: the reduction alone, 12 terms in fp32
    own = npf(jac[:V]) * g[:, :, None]
    check('se3_grad reduction', grad[:V], own.sum(1), seq_sum32(host(jac[:V]), g), np.abs(own).max(1))


# ---------------------------------------------------------------------------------------------------------------- ray generation
def reference_rays(idx, images, masks, Ks, c2w, inverse_y, normalize):
    """O.select_training_rays, and for normalize = False its per-view expression with un-normalised rays_d."""
    o, d, v, target, mask = O.select_training_rays(idx, images, masks, Ks, c2w, inverse_y=inverse_y)
    if normalize:
        return o, d, v, target, mask
    V, H, W = images.shape[:3]
    view = torch.div(idx, H * W, rounding_mode='floor')
    rem = idx - view * (H * W)
    pj = torch.div(rem, W, rounding_mode='floor')
    pi = rem - pj * W
    d_all, v_all = torch.zeros(len(idx), 3), torch.zeros(len(idx), 3)
    for k in range(V):
        sel = (view == k).nonzero()[:, 0]
        if len(sel):
            _, d, vd = O.rays_at_pixels(pi[sel], pj[sel], Ks[k], c2w[k], inverse_y=inverse_y, normalize=False)
            d_all, v_all = d_all.index_put((sel,), d), v_all.index_put((sel,), vd)
    assert torch.equal(v_all, v)
    return o, d_all, v_all, target, mask


@pytest.mark.parametrize('n_rays', [1, 255, 700])
def test_raygen_at_selected_indices_bit_exact(n_rays):
    from poseprobe_amd import ops
    from poseprobe_amd import synthetic as syn
    V, H, W = 3, 8, 12
    views = syn.make_views(V, H, W)
    images, masks, Ks = (torch.tensor(views[k]) for k in ('images', 'masks', 'Ks'))
    c2w = O.pose_invert(torch.tensor(views['w2c']))
    idx = np.random.RandomState(n_rays).randint(0, V * H * W, n_rays)             # with duplicates
    if n_rays > 2:
        idx[1] = idx[0]
        idx[-1], idx[-2] = V * H * W - 1, 0
    assert n_rays == 1 or len(np.unique(idx)) < n_rays
    intr = cu(np.stack([views['Ks'][:, 0, 0], views['Ks'][:, 1, 1], views['Ks'][:, 0, 2], views['Ks'][:, 1, 2]], -1))
    cfg = _cfg(8)
    for inverse_y in (True, False):
        for normalize in (True, False):
            ref = reference_rays(torch.tensor(idx), images, masks, Ks, c2w, inverse_y, normalize)
            o, d, vd, target = (full(n_rays + GUARD, 3) for _ in range(4))
            mask_px = full(n_rays + GUARD)
            ops.raygen_select_fwd(cfg.pp, cu(idx, torch.int32), cu(c2w), intr, H, W, inverse_y, normalize, cu(images), cu(masks),
                                  o, d, vd, target, mask_px)
            for name, got, want in zip(('rays_o', 'rays_d', 'viewdirs', 'target', 'mask_px'), (o, d, vd, target, mask_px), ref):
                untouched(name, got, n_rays)
                assert np.array_equal(host(got)[:n_rays], want.numpy().reshape(host(got)[:n_rays].shape)), \
                    (name, inverse_y, normalize)


# --------------------------------------------------------------------------------------------------------------------- samplers
def sampler_inputs(G, n_rays, kind):
    scene, cfg = scene_for(G, stepsize=0.5), _cfg(G, stepsize=0.5)
    assert cfg.n_samples == scene.n_samples()
    o, d, jit = C.sampler_rays(n_rays, kind)
    return scene, cfg, o, d, jit


@pytest.mark.parametrize('jittered', [True, False], ids=['jitter', 'nojitter'])
@pytest.mark.parametrize('G,n_rays,kind', C.SAMPLER_CASES)
def test_dense_sampler_bit_exact(G, n_rays, kind, jittered):
    """More than 64 sample slots per ray (k_sample_count / k_sample_fill carry their offset over 64-lane chunks), more than 1024
    rays (k_exclusive_scan carries its total over passes), and the rays no fixture has; against O.sample_dense + O.compact_samples
    as test_hip_kernels.py::test_dense_sampler_indices_bit_exact compares them."""
    from poseprobe_amd import ops
    scene, cfg, o, d, jit = sampler_inputs(G, n_rays, kind)
    S = cfg.n_samples
    jit_t = torch.tensor(jit) if jittered else None
    pts_r, mask_out, step_r, t_min_r, t_max_r = O.sample_dense(scene, torch.tensor(o), torch.tensor(d), jit_t)
    pts_k, rid_k, step_k_r, _ = O.compact_samples(pts_r, mask_out, step_r)
    keep_r = ~mask_out.numpy()
    M = int(keep_r.sum())
    cap = max(n_rays, M + 37)
    t_min, t_max = full(n_rays + GUARD), full(n_rays + GUARD)
    ray_start, count = ifull(n_rays + 1 + GUARD), ifull(1 + GUARD)
    pts, step, ray_id, step_k = full(cap + GUARD, 3), full(cap + GUARD), ifull(cap + GUARD), ifull(cap + GUARD)
    keep = full(n_rays * S + GUARD, value=99, dtype=torch.uint8)
    ops.sample_dense(cfg.pp, cu(o), cu(d), cu(jit) if jittered else None, cap, t_min, t_max, ray_start, count, pts, ray_id, step_k,
                     step, keep)
    assert np.array_equal(host(keep)[:n_rays * S].reshape(n_rays, S).astype(bool), keep_r)
    untouched('mask_keep', keep, n_rays * S, 99)
    assert int(count[0]) == M
    untouched('count', count, 1)
    assert np.array_equal(host(ray_start)[:n_rays + 1], np.concatenate([[0], np.cumsum(keep_r.sum(1))]))
    untouched('ray_start', ray_start, n_rays + 1)
    assert np.array_equal(host(ray_id)[:M], rid_k.numpy())
    assert np.array_equal(host(step_k)[:M], np.nonzero(keep_r)[1])
    assert np.array_equal(host(step)[:M], step_k_r.numpy())
    assert np.array_equal(host(pts)[:M], pts_k.numpy())
    assert np.array_equal(host(t_min)[:n_rays], t_min_r.numpy())
    assert np.array_equal(host(t_max)[:n_rays], t_max_r.numpy())
    for name, buf in (('pts', pts), ('step', step), ('step_k', step_k)):
        untouched(name, buf, M)
    untouched('ray_id', ray_id, max(M, n_rays))
    untouched('t_min', t_min, n_rays)
    untouched('t_max', t_max, n_rays)
    if kind == 'miss':
        assert M == 0 and (host(ray_start)[:n_rays + 1] == 0).all()


@pytest.mark.parametrize('G,n_rays,kind', C.SAMPLER_CASES)
def test_variable_sampler_bit_exact(G, n_rays, kind):
    """pp_sample_var against O.sample_variable (the C restatement of sample_pts_on_rays and the torch post-processing): per-ray step
    counts, compaction and indices exact; t_min, t_max and the points bit-equal."""
    from poseprobe_amd import ops
    scene, cfg, o, d, _ = sampler_inputs(G, n_rays, kind)
    to, td = torch.tensor(o), torch.tensor(d)
    pts_r, rid_r, sid_r, mask_out, t_min_r = O.sample_variable(scene, to, td)
    raw = native_ops.sample_pts_on_rays(to, td, scene.xyz_min, scene.xyz_max, scene.near, 1e9, float(scene.stepsize * scene.voxel_size))
    n_steps_r, t_max_r = raw[4].numpy(), raw[6].numpy()
    assert len(mask_out) == n_steps_r.sum()
    M = len(rid_r)
    per_ray = np.bincount(rid_r.numpy(), minlength=n_rays)
    cap = max(n_rays, M + 37)
    t_min, t_max = full(n_rays + GUARD), full(n_rays + GUARD)
    n_steps, ray_start, count = ifull(n_rays + GUARD), ifull(n_rays + 1 + GUARD), ifull(1 + GUARD)
    pts, ray_id, step_id = full(cap + GUARD, 3), ifull(cap + GUARD), ifull(cap + GUARD)
    ops.sample_var(cfg.pp, cu(o), cu(d), cap, t_min, t_max, n_steps, ray_start, count, pts, ray_id, step_id)
    assert np.array_equal(host(n_steps)[:n_rays], n_steps_r)
    assert int(count[0]) == M
    assert np.array_equal(host(ray_start)[:n_rays + 1], np.concatenate([[0], np.cumsum(per_ray)]))
    assert np.array_equal(host(ray_id)[:M], rid_r.numpy())
    assert np.array_equal(host(step_id)[:M], sid_r.numpy())
    assert np.array_equal(host(t_min)[:n_rays], t_min_r.numpy())
    assert np.array_equal(host(t_max)[:n_rays], t_max_r)
    assert np.array_equal(host(pts)[:M], pts_r.numpy())
    for name, buf, start in (('pts', pts, M), ('step_id', step_id, M), ('ray_id', ray_id, max(M, n_rays)), ('t_min', t_min, n_rays),
                             ('t_max', t_max, n_rays), ('n_steps', n_steps, n_rays), ('ray_start', ray_start, n_rays + 1),
                             ('count', count, 1)):
        untouched(name, buf, start)
    if kind == 'miss':
        assert M == 0


# ----------------------------------------------------------------------------------------------------------------------- losses
LOSS_PREFILL = np.array([0.5, -0.25, 3.0, 4.0, 5.0, 6.0, 0.125, 2.0], F32)
W_MAIN, W_ENT, W_MASK, W_EIK, W_DEF = 1.0, 0.01, 0.1, 1.0, 0.05


def check_added(name, got, pre, r64, r32):
    """got = pre + a sum of non-negative terms: the scale is |pre| + the sum."""
    one = lambda x: npf(x).reshape(1)
    check(name, one(got), one(pre) + one(r64), npf(F32(pre) + F32(float(r32))).reshape(1), np.abs(one(pre)) + np.abs(one(r64)))


@pytest.mark.parametrize('n_rays,loss_scale,with_norm', [(1, 1.0, False), (255, 0.1, False), (256, 1.0, False), (257, 0.1, False),
                                                         (1000, 0.25, False), (257, 0.1, True)])
def test_loss_rays_values_gradients_and_gates(n_rays, loss_scale, with_norm):
    from poseprobe_amd import ops
    r = C.ray_loss_case(n_rays)
    bn = (F32(1.7) * r['mask'].sum(), F32(123.0)) if with_norm else None
    r64, r32 = (RR.ray_losses(r['rgbm'], r['alast'], r['cw'], r['target'], r['mask'], W_MAIN, W_ENT, W_MASK, loss_scale, dtype=dt,
                              batch_norm=bn) for dt in DTYPES)
    g_rgbm, g_last, g_cw, mask_sum = full(n_rays + GUARD, 3), full(n_rays + GUARD), full(n_rays + GUARD), full(1 + GUARD)
    loss = torch.cat([cu(LOSS_PREFILL), full(GUARD)])
    ops.loss_rays(cu(r['rgbm']), cu(r['alast']), cu(r['cw']), cu(r['target']), cu(r['mask']), mask_sum, W_MAIN, W_ENT, W_MASK,
                  loss_scale, g_rgbm, g_last, g_cw, loss, None if bn is None else cu(np.array(bn, F32)))
    for name, buf in (('g_rgbm', g_rgbm), ('g_last', g_last), ('g_cw', g_cw)):
        untouched(name, buf, n_rays)
    untouched('mask_sum', mask_sum, 1)
    untouched('loss_out', loss, 8)
    assert float(mask_sum[0]) == float(r['mask'].sum()) == float(r64['mask_sum'])
    # gradients: the scale of an entry is the larger of the two terms whose difference it is
    y, a, c0 = (r[k].astype(np.float64) for k in ('mask', 'alast', 'cw'))
    norm = float(bn[0]) if with_norm else y.sum()
    s_rgbm = loss_scale * W_MAIN * 2 * np.maximum(r['rgbm'], r['target']) * y[:, None] / (norm * 3)
    p, c = np.clip(a, RR.ENT_LO, RR.ENT_HI), np.clip(c0, RR.BCE_LO, RR.BCE_HI)
    s_last = loss_scale * W_ENT * np.maximum(-np.log(p), -np.log1p(-p)) / n_rays
    s_cw = loss_scale * W_MASK * np.maximum(y / c, (1 - y) / (1 - c)) / n_rays
    check('g_rgbm', g_rgbm[:n_rays], r64['g_rgbm'], r32['g_rgbm'], s_rgbm)
    check('g_last', g_last[:n_rays], r64['g_last'], r32['g_last'], s_last)
    check('g_cw', g_cw[:n_rays], r64['g_cw'], r32['g_cw'], s_cw)
    # gates: closed (exactly 0) outside the clamp range, open at its bounds (torch's clamp backward is inclusive)
    for name, got, x, lo, hi in (('g_last', host(g_last)[:n_rays], r['alast'], F32(RR.ENT_LO), F32(RR.ENT_HI)),
                                 ('g_cw', host(g_cw)[:n_rays], r['cw'], F32(RR.BCE_LO), F32(RR.BCE_HI))):
        outside, at = (x < lo) | (x > hi), (x == lo) | (x == hi)
        assert outside.any() and (got[outside] == 0).all(), f'{name}: open outside the clamp range'
        assert (got[at] != 0).all() and (n_rays < 12 or at.sum() == 4), f'{name}: closed at a clamp bound'
    # values land on top of the prefilled ones; the sample terms' slots stay as they were
    out = host(loss)[:8]
    assert np.array_equal(out[2:6], LOSS_PREFILL[2:6])
    for slot, key in ((0, 'mse'), (1, 'entropy'), (6, 'bce'), (7, 'total')):
        check_added(f'loss_out[{slot}]', out[slot], LOSS_PREFILL[slot], r64[key], r32[key])


SAMPLE_CASES = sorted({(cap, cnt) for cap in (1, 256, 257, 1000) for cnt in (0, cap - 1, cap, cap + 5)})


@pytest.mark.parametrize('capacity,count,with_norm', [(a, b, False) for a, b in SAMPLE_CASES] + [(257, 256, True)])
def test_loss_samples_values_gradients_and_rows(capacity, count, with_norm):
    """g_gradient is accumulated (+=) into a prefilled buffer, the other three gradients are stored (=) on rows < M = min(count,
    capacity); rows >= M and, for count = 0, everything stay as they were."""
    from poseprobe_amd import ops
    s = C.sample_loss_case(capacity)
    ls = 0.1
    bn = (F32(50.0), F32(1.3 * capacity)) if with_norm else None
    args = (s['gradient'], s['grad_deform'], s['warp_out'], s['sdf_deform'], count, W_EIK, W_DEF, ls)
    r64, r32 = (RR.sample_losses(*args, dtype=dt, batch_norm=bn) for dt in DTYPES)
    M = min(count, capacity)
    assert r64['M'] == M
    rows = capacity + GUARD
    pre_g = np.random.RandomState(capacity).normal(0, 1e-3, (rows, 3)).astype(F32)
    g_gradient, g_gd, g_corr, g_sd = cu(pre_g), full(rows, 9), full(rows), full(rows)
    loss = torch.cat([cu(LOSS_PREFILL), full(GUARD)])
    ops.loss_samples(cu(s['gradient']), cu(s['grad_deform']), cu(s['warp_out']), cu(s['sdf_deform']), cu([count], torch.int32),
                     capacity, W_EIK, W_DEF, ls, g_gradient, g_gd, g_corr, g_sd, loss, None if bn is None else cu(np.array(bn, F32)))
    assert np.array_equal(host(g_gradient)[M:], pre_g[M:]), 'g_gradient: rows past count were written'
    for name, buf in (('g_grad_deform', g_gd), ('g_correction', g_corr), ('g_sdf_deform', g_sd)):
        untouched(name, buf, M)
    untouched('loss_out', loss, 8)
    out = host(loss)[:8]
    assert np.array_equal(out[[0, 1, 6]], LOSS_PREFILL[[0, 1, 6]])
    if M == 0:
        assert np.array_equal(out, LOSS_PREFILL)
        return
    # every gradient entry is one product chain: its scale is its own magnitude (plus the prefilled value it is added to)
    g64, g32 = npf(r64['g_gradient']), host(r32['g_gradient'])
    check('g_gradient', g_gradient[:M], pre_g[:M] + g64, pre_g[:M] + g32, np.abs(pre_g[:M]) + np.abs(g64))
    for name, got in (('g_grad_deform', g_gd), ('g_correction', g_corr), ('g_sdf_deform', g_sd)):
        check(name, got[:M], r64[name], r32[name], np.abs(npf(r64[name])))
        assert np.array_equal(host(got)[:M] == 0, npf(r64[name]) == 0), f'{name}: zero rows differ'
    zero_rows = (s['gradient'][:M] == 0).all(1) | (s['gradient'][:M] == (1, 0, 0)).all(1)
    assert np.array_equal(host(g_gradient)[:M][zero_rows], pre_g[:M][zero_rows]), 'zero vector / unit norm: no eikonal gradient'
    for slot, key in ((2, 'eikonal'), (3, 'grad_deform'), (4, 'correction'), (5, 'sdf_deform'), (7, 'total')):
        check_added(f'loss_out[{slot}]', out[slot], LOSS_PREFILL[slot], r64[key], r32[key])
