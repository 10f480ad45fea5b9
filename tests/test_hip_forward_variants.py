"""GPU tests of the two other branches of Voxurf.forward / Voxurf.inference: use_deform=False (plain-template geometry)
and fast_color_thres > 0 (weight-threshold compaction), against the recorded reference run, against a float64 restatement, and
against torch.nonzero; and of the default branch staying what it was."""
import numpy as np
import pytest
import torch

from tests import forward_variants_reference as R
from tests.helpers import assert_close, load

pytestmark = pytest.mark.gpu

c = lambda t: t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def golden():
    d = load('forward_variants_g24.npz')
    d.update(R.fixture_params(d))
    return d


def _model(d, thres=0.0):
    from tests.test_hip_dropin import make_model
    m = make_model(d)
    m.fast_color_thres = thres
    return m


# ------------------------------------------------------------------------------------------------ against the reference's run
@pytest.mark.parametrize('case', R.CASES)
def test_forward_and_backward_match_the_reference(golden, case):
    """Budgets: those of test_hip_dropin's forward / backward comparison at g24.  The kept set must be the reference's exactly: the
    fixture keeps every reference weight further than a relative 1e-3 from the threshold."""
    from poseprobe_amd import camera
    from poseprobe_amd import voxurf_coarse as Model
    from poseprobe_amd.losses import _AttrDict, object_losses
    d = golden
    deform, thres = R.CASE_SWITCHES[case]
    m = _model(d, thres)
    pm = Model.pose_model(i_train=np.arange(3), camera_noise=0.).cuda()
    pm.se3_refine.data.copy_(torch.tensor(d['se3']))
    w2c, c2w = camera.current_pose_c2w(pm.se3_refine, torch.tensor(d['w2c_init']).cuda())
    H, W = int(d['H']), int(d['W'])
    target, mask, ro, rd, vd = Model.select_training_rays(torch.tensor(d['ray_idx']), torch.tensor(d['images']).cuda(),
                                                          torch.tensor(d['masks']).cuda(), c2w, np.array([[H, W]] * 3), d['Ks'])
    gs = int(d['global_step'])
    out = m(ro, rd, vd, use_deform=deform, global_step=gs, jitter=torch.tensor(d['jitter']), **R.RENDER_KWARGS)
    want = set(Model.FORWARD_KEYS) | (set(Model.FORWARD_DEFORM_KEYS) if deform else set())
    assert {k for k in out if not k.startswith('_')} == want == set(d[f'{case}.keys'].tolist())
    g = lambda k: d[f'{case}.out.{k}']
    assert np.array_equal(c(out['mask']), g('mask'))
    if thres > 0:
        assert np.array_equal(np.nonzero(c(out['mask']))[0], d[f'{case}.kept']), 'kept index set'
    keys = ['alphainv_cum', 'weights', 'cum_weights', 'rgb_marched', 'raw_alpha', 'raw_rgb', 'depth', 'disp', 'gradient', 'k0_tv']
    keys += list(Model.FORWARD_DEFORM_KEYS) if deform else []
    for k in keys:
        assert out[k].shape == g(k).shape, (k, out[k].shape, g(k).shape)
        assert_close(c(out[k]), g(k), rtol=1e-4, atol=1e-5, scaled=1e-6, name=k)
    assert abs(out['s_val'] - float(g('s_val'))) < 1e-12
    cfg_train = _AttrDict(weight_main=1., weight_tv_k0=.01, weight_mask=.1)
    S, Wt, loss = object_losses(out, cfg_train, target, mask, gs, 10000, deform)
    assert_close(c(loss), d[f'{case}.loss'], rtol=1e-4, name='loss')
    (loss * 0.1).backward()
    tol = dict(rtol=1e-3, scaled=2e-5)
    gr = lambda k: d[f'{case}.grad.{k}']
    assert_close(c(pm.se3_refine.grad), gr('se3'), atol=1e-6, name='g.se3', **tol)
    gk = c(m.k0.grid.grad)[0].reshape(12, -1)
    assert_close(gk[:, d[f'{case}.k0g.voxels']].T, d[f'{case}.k0g.values'], atol=1e-9, name='g.k0 at the stored voxels', **tol)
    assert_close(np.float64(np.abs(gk.astype(np.float64)).sum()), d[f'{case}.k0g.abs_sum'], rtol=1e-4, name='sum |g.k0|')
    n_touched = int((np.abs(gk).max(0) > 0).sum())
    assert abs(n_touched - int(d[f'{case}.k0g.n_touched'])) <= 1e-3 * int(d[f'{case}.k0g.n_touched']), 'voxels with a colour-grid gradient'
    assert_close(c(m.sdf_alpha.grad), gr('sdf_alpha'), atol=1e-7, name='g.sdf_alpha', **tol)
    assert_close(c(m.sdf_beta.grad), gr('sdf_beta'), atol=1e-7, name='g.sdf_beta', **tol)
    rows = lambda t: c(t) if t.shape[0] < R.GRAD_ROW_STEP else c(t)[::R.GRAD_ROW_STEP]
    for li, lin in enumerate([m.rgbnet[0], m.rgbnet[2][0], m.rgbnet[3][0], m.rgbnet[4]]):
        assert_close(rows(lin.weight.grad), gr(f'rgbnet.{li}.weight'), atol=1e-8, name=f'g.rgbnet{li}.W', **tol)
        assert_close(c(lin.bias.grad), gr(f'rgbnet.{li}.bias'), atol=1e-8, name=f'g.rgbnet{li}.b', **tol)
    for li, lin in enumerate(m.warp_network.linears()):
        if deform:
            assert_close(rows(lin.weight.grad), gr(f'warp.{li}.weight'), atol=2e-7, name=f'g.warp{li}.W', **tol)
            assert_close(c(lin.bias.grad), gr(f'warp.{li}.bias'), atol=2e-7, name=f'g.warp{li}.b', **tol)
        else:
            assert lin.weight.grad is None and lin.bias.grad is None, 'the warp net does not run: it receives no gradient'
    assert m.sdf.grid.grad is None      # frozen template


# ------------------------------------------------------------------------------------------------ plain geometry against float64
@pytest.mark.parametrize('shape,seed', [((8, 8, 8), 1), ((6, 8, 10), 2)])
def test_plain_geometry_kernels_against_float64(shape, seed):
    """The two kernels alone.  Tolerance per quantity: 4 x the largest error of the float32 run of the restatement against its
    float64 run, at least 4 float32 ulps of the quantity's largest magnitude (R.bound).  g_pts is checked in two groups: the
    interpolant's derivative jumps at a cell face, so on lattice points the float32 and the float64 run may read neighbouring
    cells - that group's bound comes from that group alone and the other points keep the tight one."""
    from poseprobe_amd import ops
    case = R.kernel_case(shape, seed)
    r64, r32 = R.kernel_case_reference(case, torch.float64), R.kernel_case_reference(case, torch.float32)
    f = lambda t: t.float().contiguous().cuda()
    sc = ops.make_scene(case['xyz_min'].tolist(), case['xyz_max'].tolist(), list(shape), case['voxel_size'], case['stepsize'],
                        0.1, 5.0, 0.0)
    M = case['pts'].shape[0]
    cap = M + 37                                           # not a multiple of the block; rows past the count are fenced
    fence = 12345.0
    pts, ray_id = torch.zeros(cap, 3).cuda(), torch.zeros(cap, dtype=torch.int32).cuda()
    pts[:M], ray_id[:M] = f(case['pts']), case['ray_id'].int().cuda()
    count = torch.tensor([M], dtype=torch.int32).cuda()
    ab = f(torch.cat([case['sdf_alpha'], case['sdf_beta']]))
    alpha, grad, sdf_final = (torch.full(s, fence).cuda() for s in ((cap,), (cap, 3), (cap,)))
    ops.geometry_plain_fwd(sc, f(case['sdf']), ab, pts, f(case['viewdirs']), ray_id, count, cap, case['inv_s'], alpha, grad, sdf_final)
    got = dict(sdf_final=c(sdf_final), gradient=c(grad), alpha=c(alpha))
    report = []
    for k in ('sdf_final', 'gradient', 'alpha'):
        assert (got[k][M:] == fence).all(), f'{k}: rows past the count were written'
        err, b = np.abs(got[k][:M] - r64[k]).max(), R.bound(r32[k], r64[k])
        report.append(f'{k}: err {err:.3e} bound {b:.3e}')
        assert err <= b, report[-1]
    g_a, g_g = torch.zeros(cap).cuda(), torch.zeros(cap, 3).cuda()
    g_a[:M], g_g[:M] = f(case['g_alpha']), f(case['g_gradient'])
    pre = 0.5                                              # accumulate=1 adds to what the colour stage left
    g_pts, g_view, g_ab = torch.full((cap, 3), pre).cuda(), torch.full((cap, 3), pre).cuda(), torch.zeros(2).cuda()
    ops.geometry_plain_bwd(sc, f(case['sdf']), ab, pts, f(case['viewdirs']), ray_id, count, cap, case['inv_s'], g_a, g_g, None, 1,
                           g_pts, g_view, g_ab)
    assert (c(g_pts)[M:] == pre).all() and (c(g_view)[M:] == pre).all(), 'rows past the count were written'
    lat = case['lattice'].numpy()
    gp = c(g_pts)[:M].astype(np.float64) - pre
    for name, sel in (('g_pts (inside cells)', ~lat), ('g_pts (lattice points)', lat)):
        # `pre` costs the kernel's sum half an ulp of (pre + value) once more
        b = R.bound(r32['g_pts'][sel], r64['g_pts'][sel]) + R.ulp32(pre + np.abs(r64['g_pts'][sel]).max())
        err = np.abs(gp[sel] - r64['g_pts'][sel]).max()
        report.append(f'{name}: err {err:.3e} bound {b:.3e}')
        assert err <= b, report[-1]
    gv = c(g_view)[:M].astype(np.float64) - pre
    b = R.bound(r32['g_view'], r64['g_view']) + R.ulp32(pre + np.abs(r64['g_view']).max())
    assert np.abs(gv - r64['g_view']).max() <= b, f"g_view: err {np.abs(gv - r64['g_view']).max():.3e} bound {b:.3e}"
    for i, name in enumerate(('g_alpha', 'g_beta')):
        # d / d sdf_alpha, d / d sdf_beta: sums over every sample; the yardstick is the float32 run's error on the same sum
        b = R.bound(r32['g_ab'][i], r64['g_ab'][i])
        err = abs(float(g_ab[i]) - r64['g_ab'][i])
        report.append(f'{name}: err {err:.3e} bound {b:.3e} value {r64["g_ab"][i]:.6e}')
        assert err <= b, report[-1]
    print('\n'.join(report))
    # a border point passes no gradient to its clipped coordinates (F.grid_sample's border padding): the eight box corners
    assert (gp[-8:] == 0).all()


# ------------------------------------------------------------------------------------------------ compaction against torch.nonzero
def _compaction_case(lengths, thres, seed):
    g = torch.Generator().manual_seed(seed)
    M = int(sum(lengths))
    rs = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    rs[1:] = torch.tensor(lengths).cumsum(0).int()
    w = torch.rand(M, generator=g) * 2 * thres                         # about half above
    return M, rs, w


@pytest.mark.parametrize('name', ['one_ray', 'rays65'])
def test_compaction_against_nonzero(name):
    from poseprobe_amd import ops
    thres = 1e-3
    if name == 'one_ray':
        lengths = [70]                                                 # more than one wavefront's chunk
    else:
        gl = torch.Generator().manual_seed(4)
        lengths = torch.randint(1, 150, (65,), generator=gl).tolist()  # 65 rays: a second work-group row, a last work-group with one ray
        lengths[3], lengths[10], lengths[20], lengths[64] = 0, 33, 192, 192
    M, rs, w = _compaction_case(lengths, thres, 1)
    N = len(lengths)
    if name == 'rays65':
        b = rs.tolist()
        w[b[10]:b[11]] = thres * 0.5                                   # a ray keeping 0 samples
        w[b[20]:b[21]] = thres * 2                                     # a ray keeping all 192 of 192 samples
        w[b[5]] = thres                                                # exactly the threshold: not kept (strict >)
    cap = M + 50
    g = torch.Generator().manual_seed(2)
    full = lambda *s: torch.randn(cap, *s, generator=g).cuda()
    pts, step, alpha, gradient = full(3), full(), full(), full(3)
    ray_id = torch.repeat_interleave(torch.arange(N), torch.tensor(lengths)).int()
    ray_id = torch.cat([ray_id, torch.full((cap - M,), -1, dtype=torch.int32)]).cuda()
    wd = torch.cat([w, torch.full((cap - M,), 1.0)]).cuda()             # weights past the last ray would all pass: never read
    fence = -777.0
    idx, rs_k, cnt = torch.full((cap,), -777, dtype=torch.int32).cuda(), torch.full((N + 1,), -777, dtype=torch.int32).cuda(), \
        torch.full((1,), -777, dtype=torch.int32).cuda()
    pts_k, step_k, alpha_k, grad_k = (torch.full((cap, *s), fence).cuda() for s in ((3,), (), (), (3,)))
    rid_k = torch.full((cap,), -777, dtype=torch.int32).cuda()
    ops.keep_compact(wd, rs.cuda(), N, cap, thres, pts, ray_id, step, alpha, gradient, idx, rs_k, cnt, pts_k, rid_k, step_k, alpha_k, grad_k)
    want = torch.nonzero(w > thres)[:, 0]
    K = want.shape[0]
    assert int(cnt) == K and 0 < K < M
    assert torch.equal(idx[:K].cpu().long(), want)
    kept_per_ray = torch.bincount(ray_id[:M].cpu().long()[want], minlength=N)
    assert torch.equal(rs_k.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long), kept_per_ray.cumsum(0)]))
    wl = want.cuda()
    for got, src in ((pts_k, pts), (rid_k, ray_id), (step_k, step), (alpha_k, alpha), (grad_k, gradient)):
        assert torch.equal(got[:K], src[wl]), 'gathered rows'
        assert bool((got[K:] == (fence if got.dtype.is_floating_point else -777)).all()), 'rows past the kept count were written'
    assert bool((idx[K:] == -777).all())
    if name == 'rays65':
        assert kept_per_ray[3] == 0 and kept_per_ray[10] == 0 and kept_per_ray[20] == 192 and rs[6] - rs[5] > 0
    # backward: the kept rows return to their original rows, every other row is exactly zero - whatever the buffers held
    gk = [torch.randn(cap, *s, generator=g).cuda() for s in ((), (3,), (3,), (3,))]
    gf = [torch.full((cap, *s), float('nan')).cuda() for s in ((), (3,), (3,), (3,))]
    ops.keep_scatter_bwd(idx, cnt, cap, *gk, *gf)
    dropped = torch.ones(cap, dtype=torch.bool)
    dropped[want] = False
    for a, b in zip(gk, gf):
        assert torch.equal(b[wl], a[:K]) and bool((b[dropped.cuda()] == 0).all())


# ------------------------------------------------------------------------------------------------ inference paths
def test_inference_paths_with_a_threshold(golden):
    d = golden
    thres = float(d['thres'])
    m = _model(d, thres)
    ro, rd, vd = (torch.tensor(d[k]).cuda() for k in ('rays_o', 'rays_d', 'viewdirs'))
    out = m.inference(ro, rd, vd, global_step=None, **R.RENDER_KWARGS)
    K = d['inference.kept'].shape[0]
    assert out['weights'].shape[0] == out['raw_alpha'].shape[0] == out['raw_rgb'].shape[0] == out['gradient'].shape[0] == K
    assert np.array_equal(c(out['ray_id']), d['inference.ray_id']) and np.array_equal(c(out['step_id']), d['inference.step_id'])
    for k in ('alphainv_cum', 'weights', 'cum_weights', 'rgb_marched', 'normal_marched', 'raw_alpha', 'raw_rgb', 'depth', 'gradient',
              'gradient_error'):
        assert_close(c(out[k]), d['inference.out.' + k], rtol=1e-4, atol=1e-5, scaled=1e-6, name=k)
    rays = m.inference_rays(ro, rd, vd, global_step=None, **R.RENDER_KWARGS)
    for k in ('alphainv_cum', 'cum_weights', 'rgb_marched', 'depth'):
        assert torch.equal(rays[k], out[k]), k                  # the same kernels on the same samples
    assert_close(c(rays['normal_marched']), c(out['normal_marched']), rtol=1e-5, atol=1e-6, name='normal_marched')
    # a second chunk through the kept buffers of the first (fewer rays, stale rows behind them)
    sub = slice(40, 97)
    a, b = m.inference(ro[sub], rd[sub], vd[sub], **R.RENDER_KWARGS), m.inference_rays(ro[sub], rd[sub], vd[sub], **R.RENDER_KWARGS)
    for k in ('alphainv_cum', 'cum_weights', 'rgb_marched', 'depth'):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], out[k][sub]), k


# ------------------------------------------------------------------------------------------------ the default branch
def test_default_outputs_are_those_of_the_chain_without_the_switches():
    """fast_color_thres = 0 and use_deform=True: bit for bit what the default kernel chain gives when it is called directly, with
    no switch in sight (the chain RenderCore.forward ran before it had them)."""
    from poseprobe_amd import ops
    from poseprobe_amd.engine import FlatParams, Workspace
    from poseprobe_amd.grid import channels_last_view
    from tests.test_hip_dropin import make_model
    d = load('forward_g24_s7000.npz')
    m = make_model(d)
    assert m.fast_color_thres == 0
    ro, rd, vd = (torch.tensor(d[k]).cuda() for k in ('rays_o', 'rays_d', 'viewdirs'))
    jit, gs = torch.tensor(d['jitter']).cuda(), int(d['global_step'])
    with torch.no_grad():
        out = m(ro, rd, vd, use_deform=True, global_step=gs, jitter=jit, **R.RENDER_KWARGS)
        core = m._core
        cfg, sc = core.cfg, core.cfg.pp
        sb = m._sample_dense(core, ro, rd, jit)
        M = sb['M']
        cap = max((M + 4095) // 4096 * 4096, 4096)
        ws = Workspace(len(ro), cap, ro.device, backward=False, ctx=core.ctx, samples=sb)
        ws.rays_o, ws.rays_d, ws.viewdirs = ro, rd, vd
        flat = FlatParams(ro.device, moments=False)
        flat.load_reference(m.sdf_alpha, m.sdf_beta, *m._mlp_layers())
        _, inv_s = m._inv_s(gs, True)
        pe_w = m._pe_weights(cfg, gs / m.N_iters, ro.device)
        sdf = m.sdf.grid.detach()[0, 0].contiguous()
        ops.warp_fwd(flat.view('warp'), ws.pts, ws.count, cap, cfg.out_range, ws.warp_acts, ws.warp_out, core.ctx)
        ops.geometry_fwd(sc, sdf, flat.view('sdf_ab'), ws.pts, ws.warp_out, ws.viewdirs, ws.ray_id, ws.count, cap, inv_s, ws.alpha,
                         ws.gradient, ws.sdf_final, ws.sdf_deform, ws.grad_deform)
        ops.color_feat_fwd(sc, channels_last_view(m.k0.grid), ws.pts, ws.viewdirs, ws.ray_id, ws.gradient, pe_w, ws.count, cap, ws.feat)
        ops.rgbnet_fwd(flat.view('rgbnet'), ws.feat, ws.count, cap, ws.rgb_acts, ws.rgb, core.ctx)
        ops.march_fwd(ws.alpha, ws.rgb, ws.step, None, ws.ray_start, ws.N, cfg.bg, ws.weights, ws.T, ws.alphainv_last, ws.i_end,
                      ws.rgb_marched, ws.rgb_pre, ws.cum_weights, ws.depth_acc, None)
    assert out['weights'].shape[0] == M
    for k, t in (('raw_alpha', ws.alpha[:M]), ('gradient', ws.gradient[:M]), ('weights', ws.weights[:M]), ('raw_rgb', ws.rgb[:M]),
                 ('rgb_marched', ws.rgb_marched), ('alphainv_cum', ws.alphainv_last), ('sdf_deform', ws.sdf_deform[:M]),
                 ('grad_deform', ws.grad_deform[:M].reshape(M, 3, 3)), ('sdf_correct', ws.warp_out[:M, 3:4]), ('_n_step', ws.depth_acc)):
        assert torch.equal(out[k], t), k
    from poseprobe_amd import voxurf_coarse as Model
    assert tuple(out) == Model.FORWARD_KEYS + Model.FORWARD_DEFORM_KEYS + ('_t_min', '_n_step')


# ------------------------------------------------------------------------------------------------ surface query
def _composite(alpha, ray_start):
    """Alphas2Weights restated in torch (float64-capable, differentiable): w_i = T_i alpha_i with the 1e-3 early stop."""
    ws = []
    for b, e in zip(ray_start[:-1], ray_start[1:]):
        a = alpha[b:e]
        T = torch.cat([torch.ones(1, dtype=a.dtype), torch.cumprod(1 - a, 0)])
        live = torch.cat([torch.ones(1, dtype=torch.bool), (T[1:-1] >= 1e-3).cumprod(0).bool()]) if e > b else torch.ones(0, dtype=torch.bool)
        ws.append(T[:-1] * a * live)
    return torch.cat(ws) if ws else alpha[:0]


def test_surface_query_without_the_warp_net_against_float64_autograd(golden):
    """query_sdf_point_wocuda_render(use_deform=False, keep_dim=True): points and depth, and the gradient of a random functional of
    the points w.r.t. the rays, against autograd through the float64 restatement on the kernel's own sample slots.  Tolerance:
    4 x the float32 run of the same restatement against its float64 run, floor 4 ulps (R.bound)."""
    d = golden
    m = _model(d, thres=1e-3)                      # the query composites every sample whatever the threshold is
    gs = int(d['global_step'])
    sub = slice(0, 96)
    ro = torch.tensor(d['rays_o'][sub]).cuda().requires_grad_(True)
    rd = torch.tensor(d['rays_d'][sub]).cuda().requires_grad_(True)
    jit = torch.tensor(d['jitter'][sub]).cuda()
    gen = torch.Generator().manual_seed(0)
    wsum = torch.randn(96, 3, generator=gen, dtype=torch.float64)
    pts, hit, depth = m.query_sdf_point_wocuda_render(ro, rd, global_step=gs, keep_dim=True, use_deform=False, jitter=jit,
                                                      **R.RENDER_KWARGS)
    (pts * wsum.float().cuda()).sum().backward()
    for lin in m.warp_network.linears():
        assert lin.weight.grad is None
    core = m._core
    with torch.no_grad():
        sb = m._sample_dense(core, ro.detach(), rd.detach(), jit)
    M = sb['M']
    ray_id, step, rs = sb['ray_id'][:M].cpu().long(), sb['step'][:M].cpu(), sb['ray_start'].cpu().tolist()
    P = {k: torch.tensor(d[k]) for k in ('P.sdf', 'P.sdf_alpha', 'P.sdf_beta')}
    scene_min, scene_max = m.xyz_min.cpu(), m.xyz_max.cpu()

    def restated(dtype):
        t = lambda x: x.detach().cpu().to(dtype)
        o, dd = t(ro).requires_grad_(True), t(rd).requires_grad_(True)
        nrm = dd.norm(dim=-1)
        vec = torch.where(dd == 0, torch.full_like(dd, 1e-6), dd)
        t_min = torch.minimum((t(scene_max) - o) / vec, (t(scene_min) - o) / vec).amax(-1).clamp(min=R.RENDER_KWARGS['near'],
                                                                                                  max=R.RENDER_KWARGS['far'])
        x = o[ray_id] + dd[ray_id] * (t_min[ray_id] + t(step) / nrm[ray_id])[:, None]
        dirs = (dd / nrm[:, None])[ray_id]
        _, _, alpha = R.plain_geometry(t(P['P.sdf'])[0, 0], t(P['P.sdf_alpha']), t(P['P.sdf_beta']), x, dirs, t(scene_min), t(scene_max),
                                       torch.tensor(core.cfg.voxel_size, dtype=dtype), torch.tensor(core.cfg.step_dist, dtype=dtype),
                                       torch.tensor(core.cfg.inv_s(gs), dtype=dtype))
        w = _composite(alpha, rs)
        n_step = torch.zeros(96, dtype=dtype).index_add(0, ray_id, w * t(step))
        dep = t_min + n_step / nrm
        p = o + dd * dep[:, None]
        (p * wsum.to(dtype)).sum().backward()
        n = lambda z: z.detach().double().numpy()
        return dict(pts=n(p), depth=n(dep), g_o=n(o.grad), g_d=n(dd.grad), hit=(n_step > 0).numpy())

    r64, r32 = restated(torch.float64), restated(torch.float32)
    assert np.array_equal(c(hit), r64['hit']) and r64['hit'].any() and not r64['hit'].all()
    for k, got in (('pts', pts), ('depth', depth[:, 0]), ('g_o', ro.grad), ('g_d', rd.grad)):
        err, b = np.abs(c(got) - r64[k]).max(), R.bound(r32[k], r64[k])
        print(f'{k}: err {err:.3e} bound {b:.3e}')
        assert err <= b, f'{k}: err {err:.3e} bound {b:.3e}'
