"""Engine-native reprojection + near-surface pass (TrainEngine.reprojection_grads, csrc/pp_reproj.hip): parity with the
reference's recorded get_project_error in both modes, the parameter gradients of the render mode against autograd through the
drop-in module, the loss kernel alone against a float64 restatement, a buffer fence around the new kernels, and the joint step."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close, load, params_from_npz

pytestmark = pytest.mark.gpu

GS = 50                     # the global step the fixture was recorded at
RK = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, flip_x=False, flip_y=False)


def _engine(d, reproj_rows=192, n_rand=64, **kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    rs = syn.range_shape()
    G, H, W = int(d['G']), int(d['H']), int(d['W'])
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max()))
    eng = TrainEngine(cfg, 3, H, W, n_rand, reproj_rows=reproj_rows, **kw)
    eng.set_views(np.zeros((3, H, W, 3), np.float32), np.ones((3, H, W, 1), np.float32), d['Ks'], d['w2c_init'])
    P = params_from_npz(d)
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'], se3=torch.tensor(d['se3']))
    eng.zero_grads()
    return eng


def _rows(d, dev='cuda'):
    """Both pairs of the fixture at once, in get_project_error's row order: [coord0 of every pair | coord1 of every pair]."""
    it, jt = d['i_train'], d['j_train']
    n = d['coord0'].shape[1]
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    return dict(own=t(np.repeat(np.concatenate([it, jt]), n), torch.int32), other=t(np.repeat(np.concatenate([jt, it]), n), torch.int32),
                pix=t(np.concatenate([d['coord0'], d['coord1']]).reshape(-1, 2), torch.float32),
                match=t(np.concatenate([d['coord1'], d['coord0']]).reshape(-1, 2), torch.float32),
                conf=t(np.concatenate([d['mconf'], d['mconf']]).reshape(-1), torch.float32))


def _main_pass(eng):
    """The step's own pass (pose, BARF weights), then clean gradient buffers: what is left afterwards is the pass's share."""
    g = torch.Generator().manual_seed(0)
    ray_idx = torch.randperm(3 * eng.H * eng.W, generator=g)[:eng.N].to(torch.int32).cuda()
    eng.render_and_grads(ray_idx, torch.rand(eng.N, generator=g).cuda(), GS)
    eng.zero_grads()


def _native(d, mode, reproj_rows=192, **kw):
    eng = _engine(d, reproj_rows=reproj_rows)
    _main_pass(eng)
    eng.reprojection_grads(_rows(d), mode, GS, jitter=torch.tensor(d['jitter']).cuda(), nl=float(d['nl']), pixel_thre=200, scale=1.0, **kw)
    torch.cuda.synchronize()
    return eng


def _autograd(d, model, use_deform):
    """recon_utils.get_project_error on `model` through autograd, as tests/test_recon_utils.py calls it."""
    from poseprobe_amd import camera
    from poseprobe_amd import recon_utils as R
    dev = 'cuda'
    se3 = torch.tensor(d['se3'], device=dev, requires_grad=True)
    init = torch.tensor(d['w2c_init'], device=dev)
    w2c = torch.cat([init[:1], camera.pose.compose([camera.lie.se3_to_SE3(se3), init])[1:]], 0)
    err, near = R.get_project_error(model, torch.tensor(d['Ks'], device=dev), np.array([[int(d['H']), int(d['W'])]] * 3), float(d['nl']),
                                    GS, w2c, torch.tensor(d['coord0'], device=dev), torch.tensor(d['coord1'], device=dev),
                                    d['i_train'], d['j_train'], torch.tensor(d['mconf'], device=dev), use_deform=use_deform,
                                    pixel_thre=200, jitter=torch.tensor(d['jitter']), **RK)
    return err, near, se3, w2c


@pytest.mark.parametrize('reproj_rows', [192, 200])
@pytest.mark.parametrize('mode', ['render', 'crossing'])
def test_pass_matches_the_reference(mode, reproj_rows):
    """err, near and d (err + near) / d se3 of the native pass == what the reference's get_project_error produced (fixture), with
    the tolerances of test_recon_utils.test_project_error_matches_reference.  reproj_rows = 200: the fixture's 192 rows on a larger
    capacity - eight rays that miss the box and a zero-padded jitter go through the whole chain; same expectations, nothing but
    finite values in the parameter gradients."""
    d = load('reproj_g24.npz')
    eng = _native(d, mode, reproj_rows=reproj_rows)
    assert bool(torch.isfinite(eng.flat.grad).all()) and bool(torch.isfinite(eng.se3_grad).all())
    assert eng.ws_reproj.N == reproj_rows and int(eng.ws_reproj.ray_start[192]) == int(eng.ws_reproj.ray_start[reproj_rows])
    tag = 'deform' if mode == 'render' else 'plain'
    t = eng.last_reproj_terms
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t.values())
    print(f"{mode}: err {float(t['err']):.7g} (ref {float(d[f'err_{tag}']):.7g}) near {float(t['near']):.7g} "
          f"(ref {float(d[f'near_{tag}']):.7g}) n_valid {float(t['n_valid'])}")
    print('se3 grad', eng.se3_grad.cpu().numpy(), 'ref', d[f'g_se3_{tag}'])
    assert_close(np.float32(t['err'].item()), d[f'err_{tag}'], rtol=2e-4, atol=1e-5, name='projection_dis_error')
    assert_close(np.float32(t['near'].item()), d[f'near_{tag}'], rtol=1e-5, atol=1e-5, name='near_surface_loss')
    assert_close(eng.se3_grad.cpu().numpy(), d[f'g_se3_{tag}'], rtol=2e-3, atol=1e-4, scaled=1e-3, name='d/d se3')


def test_render_mode_reaches_the_warp_network_and_alpha_beta():
    """flat.grad of the render mode == autograd of get_project_error on engine.voxurf_view() (the route
    test_backward_is_complete_over_every_output_of_the_forward_dict pins against the reference; its tolerances); the colour grid's
    gradient and its touch marks stay exactly as they were.  The crossing mode reads the raw template only: flat.grad stays 0."""
    d = load('reproj_g24.npz')
    eng = _engine(d)
    _main_pass(eng)
    g = torch.Generator().manual_seed(1)
    eng.k0_grad.copy_(torch.randn(eng.k0_grad.shape, generator=g))
    eng.k0_touched.copy_(torch.randint(0, 2, eng.k0_touched.shape, generator=g).to(torch.uint8))
    k0_grad, touched = eng.k0_grad.clone(), eng.k0_touched.clone()
    kw = dict(jitter=torch.tensor(d['jitter']).cuda(), nl=float(d['nl']), pixel_thre=200, scale=1.0)
    eng.reprojection_grads(_rows(d), 'crossing', GS, **kw)
    assert float(eng.flat.grad.abs().max()) == 0.0 and float(eng.se3_grad.abs().max()) > 0
    eng.se3_grad.zero_()
    eng.reprojection_grads(_rows(d), 'render', GS, **kw)
    torch.cuda.synchronize()
    assert torch.equal(eng.k0_grad, k0_grad) and torch.equal(eng.k0_touched, touched)
    model = eng.voxurf_view()
    err, near, se3, _ = _autograd(d, model, True)
    (err + near).backward()
    tol = dict(rtol=2e-3, atol=1e-5, scaled=1e-3)
    assert_close(eng.se3_grad, se3.grad, name='d/d se3', **tol)
    P = dict(model.named_parameters())
    got = eng.flat.export_grads()
    assert float(eng.flat.view('warp', 'grad').abs().max()) > 0
    for i, (W, b) in enumerate(got['warp']):
        for t, key in ((W, 'weight'), (b, 'bias')):
            ref = P[f'warp_network.deform_net.net.net.{i}.0.{key}'].grad
            print(f'warp.{i}.{key}: max |ref| {float(ref.abs().max()):.3e} max |err| {float((t - ref).abs().max()):.3e}')
            assert_close(t, ref, name=f'warp.{i}.{key}', **tol)
    for key in ('sdf_alpha', 'sdf_beta'):
        print(key, float(got[key]), float(P[key].grad))
        assert_close(got[key], P[key].grad, name=key, **tol)
    assert float(got['sdf_alpha'].abs()) > 0 or float(got['sdf_beta'].abs()) > 0


@pytest.mark.parametrize('mode', ['render', 'crossing'])
def test_surface_points_agree_with_the_module_row_by_row(mode):
    """The pass's surface points and hit flags against the drop-in module's queries on the same rays and jitter.  Rows whose hit
    flags differ (a sample within rounding distance of a sign change or of the box) are excluded; at most 1 % may."""
    d = load('reproj_g24.npz')
    eng = _native(d, mode)
    ws = eng.ws_reproj
    model = eng.voxurf_view()
    jit = torch.tensor(d['jitter']).cuda()
    with torch.no_grad():
        if mode == 'render':
            pts, hit, _ = model.query_sdf_point_wocuda_render(ws.rays_o, ws.rays_d, global_step=GS, keep_dim=True, jitter=jit, **RK)
            acc = ws.depth_acc
            p, h = ws.rays_o + ws.rays_d * (ws.t_min + acc)[:, None], acc > 0
        else:
            pts, hit, _ = model.query_sdf_point_wocuda_wodeform(ws.rays_o, ws.rays_d, global_step=GS, keep_dim=True, jitter=jit, **RK)
            p, h = eng._rp['p'], eng._rp['hit'].bool()
    same = hit.bool() == h
    print(f'{mode}: {int((~same).sum())} of {same.numel()} hit flags differ, {int(h.sum())} hits')
    assert float((~same).float().mean()) <= 0.01
    assert 0 < int(h.sum())
    keep = same & h
    assert_close(p[keep], pts[keep], rtol=1e-5, atol=1e-5, name='surface points')


# ---------------------------------------------------------------------------------------------------------------------------
# the loss kernel alone
CATS = ('behind', 'miss', 'conf0', 'beyond', 'valid')
INTR = [[40., 42., 16., 15.], [38., 38., 15.5, 16.5], [44., 40., 17., 16.]]
CENTRE, HALF, NL, THRE = (0.1, -0.05, 0.2), 0.3, 0.05, 20.0


def _poses():
    """Three cameras on a circle of radius 2 looking at the origin (w2c, [3,3,4])."""
    out = []
    for a in (0.0, 0.5, -0.6):
        c = np.array([2 * np.sin(a), 0.2 * a, -2 * np.cos(a)])
        z = -c / np.linalg.norm(c)
        x = np.cross([0., 1., 0.], z); x /= np.linalg.norm(x)
        y = np.cross(z, x)
        R = np.stack([x, y, z])                      # rows: camera axes in world coordinates
        out.append(np.concatenate([R, (-R @ c)[:, None]], 1))
    return torch.tensor(np.stack(out), dtype=torch.float32)


def _loss_problem(n, render, seed):
    """Rows built so that every category of the mask is populated (r % 6: behind the near plane, miss, conf = 0, beyond
    pixel_thre, valid, valid), with wide margins: fp32 and fp64 decide every row alike."""
    g = torch.Generator().manual_seed(seed)
    w2c, K = _poses(), torch.tensor(INTR)
    own = torch.randint(0, 3, (n,), generator=g)
    other = (own + 1 + torch.randint(0, 2, (n,), generator=g)) % 3
    cat = torch.arange(n) % 6
    Rw, tw = w2c[:, :, :3], w2c[:, :, 3]
    centre_cam = -(Rw.transpose(1, 2) @ tw[:, :, None])[:, :, 0]                     # camera centres
    o = centre_cam[own]
    p = (torch.rand(n, 3, generator=g) - 0.5) * 0.8                                    # near the origin: in front of every camera
    back = cat == 0                                                                    # behind the OTHER camera's near plane
    zax = Rw[other][:, 2]
    p[back] = (centre_cam[other] - zax * (0.3 + torch.rand(n, 1, generator=g)))[back]
    q = (Rw[other] @ p[:, :, None])[:, :, 0] + tw[other]
    Ko = K[other]
    proj = torch.stack([Ko[:, 0] * q[:, 0] / q[:, 2] + Ko[:, 2], Ko[:, 1] * q[:, 1] / q[:, 2] + Ko[:, 3]], -1)
    ang = torch.rand(n, generator=g) * 6.283
    rad = torch.where(torch.arange(n) % 12 < 6, 0.2 + 0.6 * torch.rand(n, generator=g), 2.0 + 6.0 * torch.rand(n, generator=g))
    rad = torch.where(cat == 3, 60.0 + 40.0 * torch.rand(n, generator=g), rad)         # both Huber branches; beyond the threshold
    match = proj + rad[:, None] * torch.stack([ang.cos(), ang.sin()], -1)
    match[back] = torch.rand(int(back.sum()), 2, generator=g) * 31
    conf = 0.2 + torch.rand(n, generator=g)
    conf[cat == 2] = 0.0
    hit = (cat != 1).to(torch.uint8)
    depth = (p - o).norm(dim=1)
    d = (p - o) / depth[:, None]
    flip = (torch.arange(n) % 12 == 1)                                                 # among the misses: the centre lies behind the ray
    d[flip] = -d[flip]
    t_min = (0.25 + 0.2 * torch.rand(n, generator=g)) * depth
    acc = depth - t_min
    acc[cat == 1] = 0.0
    rows = dict(own=own.int(), other=other.int(), match=match, conf=conf, o=o, d=d, p=p, hit=hit, t_min=t_min, acc=acc)
    return rows, w2c, K, cat


def _loss_reference(rows, w2c, K, render, w_near, w_proj, scale):
    """The issue's formula in float64 torch; returns the scalars, the categories it saw and the gradients by autograd."""
    f = lambda t: t.double().clone()
    o, d = f(rows['o']).requires_grad_(True), f(rows['d']).requires_grad_(True)
    W = f(w2c).requires_grad_(True)
    other = rows['other'].long()
    if render:
        depth = (f(rows['t_min']) + f(rows['acc'])).requires_grad_(True)
        p = o + d * depth[:, None]
        p.retain_grad()
        h = rows['acc'].double() > 0
    else:
        depth = None
        p = f(rows['p']).requires_grad_(True)
        h = rows['hit'].bool()
    c = f(rows['conf'])
    s = torch.tensor(CENTRE, dtype=torch.float64) - o
    t = (s * d).sum(1)
    dist = torch.where(t < 0, s.norm(dim=1), (s - t[:, None] * d).norm(dim=1))
    near = (torch.clamp(dist - HALF, min=0.0) * (c > 0)).sum()
    q = (W[other][:, :, :3] @ p[:, :, None])[:, :, 0] + W[other][:, :, 3]
    behind = q[:, 2] < NL
    q = torch.where(behind[:, None], torch.full_like(q, NL), q)
    Ko = K.double()[other]
    uv = torch.stack([Ko[:, 0] * q[:, 0] / q[:, 2] + Ko[:, 2], Ko[:, 1] * q[:, 1] / q[:, 2] + Ko[:, 3]], -1)
    e = (uv - f(rows['match'])).norm(dim=1)
    valid = ~behind & h & (e.detach() <= THRE)
    hub = torch.where(e < 1, 0.5 * e * e, e - 0.5)
    err = (valid * c * hub).sum() / (valid.sum() + 1e-6)
    (scale * (w_near * near + w_proj * err)).backward()
    seen = dict(behind=behind, miss=~h, conf0=c == 0, beyond=~behind & h & (e.detach() > THRE), valid=valid,
                near_on=(dist.detach() > HALF) & (c > 0), near_back=t.detach() < 0, small=valid & (e.detach() < 1),
                large=valid & (e.detach() > 1))
    z = torch.zeros_like
    return dict(err=err.detach(), near=near.detach(), n_valid=valid.sum().double(), g_p=p.grad, g_o=o.grad, g_d=d.grad,
                g_depth=z(c) if depth is None else depth.grad, g_w2c=W.grad, seen=seen)


@pytest.mark.parametrize('render', [False, True])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 257, 1500])
def test_loss_kernel_equals_a_float64_restatement(n, render):
    """pp_reproj_loss: the three scalars, the per-row gradients and the w2c gradient against float64 autograd over the formula,
    at the tolerances tests/test_hip_scene_corres.py uses for its loss kernels (fp32 against a higher-precision reference).
    capacity = n + 7: the padding rows of every input hold NaN and must neither be read nor leave anything but zeros."""
    from poseprobe_amd import ops
    rows, w2c, K, cat = _loss_problem(n, render, seed=n)
    w_near, w_proj, scale = 0.1, 0.7, 0.5
    ref = _loss_reference(rows, w2c, K, render, w_near, w_proj, scale)
    if n >= 63:
        for k in CATS + ('near_on', 'near_back', 'small', 'large'):
            assert int(ref['seen'][k].sum()) >= 5, (k, int(ref['seen'][k].sum()))
    cap = n + 7

    def padded(t, fill=float('nan')):
        # view index 1 and hit = 1 past n_rows: a kernel that walked to `capacity` would add these NaN rows to its sums
        fill = fill if t.is_floating_point() else 1
        out = torch.full((cap,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        out[:n] = t
        return out.cuda().contiguous()
    dev = {k: padded(v) for k, v in rows.items()}
    nan = lambda *s: torch.full(s, float('nan'), device='cuda')
    terms, g_p, g_depth, g_o, g_d, g_w2c = nan(3), nan(cap, 3), nan(cap), nan(cap, 3), nan(cap, 3), nan(3, 3, 4)
    ops.reproj_loss(render, n, dev['other'], dev['match'], dev['conf'], dev['o'], dev['d'], None if render else dev['p'],
                    None if render else dev['hit'], dev['t_min'] if render else None, dev['acc'] if render else None, K.cuda(),
                    w2c.cuda(), CENTRE, HALF, NL, THRE, w_near, w_proj, scale, terms, g_p, g_depth, g_o, g_d, g_w2c)
    torch.cuda.synchronize()
    what = f'n={n} render={render}'
    for t in (terms, g_p, g_depth, g_o, g_d, g_w2c):
        assert bool(torch.isfinite(t).all()), what
    for t in (g_p, g_depth, g_o, g_d):
        assert float(t[n:].abs().max()) == 0.0, 'padding rows ' + what
    print(what, 'err', float(terms[0]), float(ref['err']), 'near', float(terms[1]), float(ref['near']), 'n_valid', float(terms[2]))
    assert float(terms[2]) == float(ref['n_valid'])
    assert_close(terms[0], ref['err'], rtol=2e-5, atol=1e-9, name='err ' + what)
    assert_close(terms[1], ref['near'], rtol=2e-5, atol=1e-9, name='near ' + what)
    for got, key in ((g_p, 'g_p'), (g_depth, 'g_depth'), (g_o, 'g_o'), (g_d, 'g_d')):
        assert_close(got[:n], ref[key], rtol=1e-4, atol=1e-10, scaled=1e-5, name=f'{key} {what}')
    assert_close(g_w2c, ref['g_w2c'], rtol=1e-3, atol=1e-10, scaled=1e-4, name='g_w2c ' + what)
    if n >= 63:
        assert float(g_w2c.abs().max()) > 0 and float(g_p.abs().max()) > 0
        assert float(g_p[:n][(cat == 2)].abs().max()) == 0.0                       # conf = 0 rows: counted, no gradient


def test_rays_and_pose_fold_equal_torch():
    """pp_reproj_rays == recon_utils.get_ray_dir (mode 'no_center') per row; pp_reproj_pose_fold == autograd of a linear functional
    of (rays_o, rays_d, t_min, w2c) w.r.t. c2w, the slab test differentiated by torch (Voxurf._entry_distance's algebra)."""
    from poseprobe_amd import ops, recon_utils as R
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig
    rs = syn.range_shape()
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, 24 ** 3, out_range=float(rs.max()))
    g = torch.Generator().manual_seed(4)
    n, cap, V = 301, 320, 3
    w2c = _poses()
    c2w = torch.cat([w2c[:, :, :3].transpose(1, 2), -(w2c[:, :, :3].transpose(1, 2) @ w2c[:, :, 3:])], -1).contiguous()
    K = torch.tensor(INTR)
    own = torch.randint(0, V, (n,), generator=g)
    pix = torch.rand(n, 2, generator=g) * 31
    ro, rd, vd = (torch.full((cap, 3), float('nan'), device='cuda') for _ in range(3))
    ops.reproj_rays(cfg.pp, own.int().cuda(), pix.cuda(), n, K.cuda(), c2w.cuda(), ro, rd, vd)
    Km = torch.zeros(V, 3, 3)
    Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2], Km[:, 2, 2] = K[:, 0], K[:, 1], K[:, 2], K[:, 3], 1.
    c = c2w.double().clone().requires_grad_(True)
    o, d = R.get_ray_dir(pix.double()[:, None], Km.double()[own], c[own], True, False, False, mode='no_center')
    o, d = o[:, 0], d[:, 0]
    assert_close(ro[:n], o.detach(), rtol=1e-6, atol=1e-7, name='rays_o')
    assert_close(rd[:n], d.detach(), rtol=1e-5, atol=1e-6, name='rays_d')
    assert torch.equal(rd, vd) and bool(torch.isfinite(ro).all())
    # rows past n_rows: rays that miss the box
    lo, hi = torch.tensor(syn.XYZ_MIN).double(), torch.tensor(syn.XYZ_MAX).double()
    assert bool((ro[n:].cpu().double() > hi).all()) and bool((rd[n:].cpu() == torch.tensor([0., 0., 1.])).all())
    go, gd, gv = (torch.randn(n, 3, generator=g) for _ in range(3))
    gt, g_w2c = torch.randn(n, generator=g), torch.randn(V, 3, 4, generator=g)
    vec = torch.where(d == 0, torch.full_like(d, 1e-6), d)
    t_min = torch.minimum((hi - o) / vec, (lo - o) / vec).amax(-1).clamp(min=cfg.near, max=cfg.far)
    assert 0.2 < float(((t_min > cfg.near) & (t_min < cfg.far)).double().mean())           # the slab test is live
    w2c_of_c = torch.cat([c[:, :, :3].transpose(1, 2), -(c[:, :, :3].transpose(1, 2) @ c[:, :, 3:])], -1)
    ((o * go.double()).sum() + (d * (gd + gv).double()).sum() + (t_min * gt.double()).sum() + (w2c_of_c * g_w2c.double()).sum()).backward()
    out = torch.full((V, 3, 4), float('nan'), device='cuda')
    ops.reproj_pose_fold(cfg.pp, own.int().cuda(), pix.cuda(), n, K.cuda(), c2w.cuda(), w2c.cuda(), ro, rd, go.cuda(), gd.cuda(),
                         gv.cuda(), gt.cuda(), g_w2c.cuda(), out)
    assert_close(out, c.grad, rtol=1e-4, atol=1e-5, scaled=1e-5, name='g_c2w')


def test_new_kernels_stay_inside_their_buffers():
    """Every buffer the new kernels write sits in a 64 KB-sentineled arena, at 1, 512 and 1500 rows (capacity = rows + 3).  Run
    once per case, no repetition."""
    from poseprobe_amd import ops
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig
    rs = syn.range_shape()
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, 24 ** 3, out_range=float(rs.max()))
    S = cfg.n_samples
    PAD, SENT = 16384, 0x7FC0DEAD

    def fenced(*shape):
        n = int(np.prod(shape))
        arena = torch.empty(n + 2 * PAD, dtype=torch.int32, device='cuda').fill_(SENT).view(torch.float32)
        return (arena, n), arena[PAD:PAD + n].view(*shape)

    def intact(fence, what):
        arena, n = fence
        a = arena.view(torch.int32)
        assert bool((a[:PAD] == SENT).all()) and bool((a[PAD + n:] == SENT).all()), what

    for n in (1, 512, 1500):
        cap = n + 3
        rows, w2c, K, _ = _loss_problem(n, True, seed=n)
        c2w = torch.cat([w2c[:, :, :3].transpose(1, 2), -(w2c[:, :, :3].transpose(1, 2) @ w2c[:, :, 3:])], -1).contiguous().cuda()
        w2c, K = w2c.cuda(), K.cuda()
        R_ = {k: v.cuda().contiguous() for k, v in rows.items()}
        pix = (torch.rand(n, 2) * 31).cuda()
        fences = {}
        for name, shape in (('ro', (cap, 3)), ('rd', (cap, 3)), ('vd', (cap, 3)), ('pts', (cap * S, 3)), ('terms', (3,)), ('g_p', (cap, 3)),
                            ('g_depth', (cap,)), ('g_o', (cap, 3)), ('g_d', (cap, 3)), ('g_w2c', (3, 3, 4)), ('g_c2w', (3, 3, 4))):
            fences[name] = fenced(*shape)
        B = {k: v[1] for k, v in fences.items()}
        ops.reproj_rays(cfg.pp, R_['own'], pix, n, K, c2w, B['ro'], B['rd'], B['vd'])
        t_min = torch.rand(cap).cuda()
        ops.reproj_dense_pts(cfg.pp, B['ro'], B['rd'], t_min, torch.rand(cap).cuda(), B['pts'])
        ops.reproj_loss(True, n, R_['other'], R_['match'], R_['conf'], R_['o'], R_['d'], None, None, R_['t_min'], R_['acc'], K, w2c,
                        CENTRE, HALF, NL, THRE, 0.1, 1.0, 1.0, B['terms'], B['g_p'], B['g_depth'], B['g_o'], B['g_d'], B['g_w2c'])
        ops.reproj_pose_fold(cfg.pp, R_['own'], pix, n, K, c2w, w2c, B['ro'], B['rd'], B['g_o'], B['g_d'], B['g_p'], B['g_depth'],
                             B['g_w2c'], B['g_c2w'])
        torch.cuda.synchronize()
        for name, (fence, buf) in fences.items():
            intact(fence, f'n={n} {name}')
            assert bool(torch.isfinite(buf).all()), f'n={n} {name}'


# ---------------------------------------------------------------------------------------------------------------------------
def _joint(d, opt):
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.joint import DualBranchEngine
    torch.manual_seed(5)
    net = bg_nerf.NeRF(opt, device='cuda')
    net.progress.data.fill_(0.6)
    eng = _engine(d)
    return eng, DualBranchEngine(eng, net, depth_range=(0.5, 3.0))


@pytest.mark.parametrize('mode', ['render', 'crossing'])
def test_joint_step_adds_the_scaled_share_and_nothing_else(mode):
    """forward_backward(reproj=...): se3_grad = the step without the term + loss_scale * the pass's share; the scene network's
    gradient block is the one of the step without it; a second call with the same inputs reproduces last_reproj_terms and what the
    new kernels wrote bit for bit.  Tolerance of the two comparisons across runs: the object and scene branches end in float
    atomics, whose order moves a sum by a few ulp of its largest term - 1e-5 of the largest entry, + 1e-4 relative."""
    from poseprobe_amd import bg_nerf
    d = load('reproj_g24.npz')
    opt = bg_nerf.default_options(sample_intvs=16)
    g = torch.Generator().manual_seed(3)
    V, N, S, H, W = 3, 24, 16, int(d['H']), int(d['W'])
    ray_idx = torch.randperm(V * H * W, generator=g)[:64].to(torch.int32).cuda()
    jitter = torch.rand(64, generator=g).cuda()
    pixels = (torch.rand(N, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda()
    image, rand = torch.rand(V, N, 3, generator=g).cuda(), torch.rand(V, N, S, 1, generator=g).cuda()
    rp = dict(rows=_rows(d), mode=mode, weight_projection=0.3, weight_near_surface=0.2, nl=float(d['nl']), pixel_thre=200,
              jitter=torch.tensor(d['jitter']).cuda())
    runs = []
    for reproj in (None, rp, rp):
        eng, joint = _joint(d, opt)
        extra = {} if reproj is None else {'reproj': reproj}
        joint.forward_backward(ray_idx, jitter, GS, pixels, image, depth_rand=rand, **extra)
        torch.cuda.synchronize()
        runs.append((eng, joint.scene.states[0].grad.clone()))
    (e0, s0), (e1, s1), (e2, s2) = runs
    # the pass's share on its own, unscaled
    e0.zero_grads()
    e0.reprojection_grads(rp['rows'], mode, GS, jitter=rp['jitter'], weight_projection=0.3, weight_near_surface=0.2, nl=rp['nl'],
                          pixel_thre=200, scale=1.0)
    share = e0.se3_grad.clone()
    assert float(share.abs().max()) > 0 and float(share[0].abs().max()) == 0.0           # view 0 is not refined
    # re-run the step without the term for its pose gradient (zero_grads above cleared it)
    eb, jb = _joint(d, opt)
    jb.forward_backward(ray_idx, jitter, GS, pixels, image, depth_rand=rand)
    tol = dict(rtol=1e-4, atol=0, scaled=1e-5)
    assert_close(e1.se3_grad, eb.se3_grad + e1.loss_scale * share, name='se3_grad', **tol)
    assert_close(s1, s0, name='scene gradient block', **tol)
    assert_close(e1.k0_grad, eb.k0_grad, name='k0_grad', **tol)
    for k in ('err', 'near', 'n_valid'):
        assert torch.equal(e1.last_reproj_terms[k], e2.last_reproj_terms[k]), k
    same = ('g_p', 'g_w2c', 'g_o', 'g_d', 'g_depth') + (('g_c2w', 'go', 'gd', 'g_t') if mode == 'crossing' else ())
    for k in same:
        assert torch.equal(e1._rp[k], e2._rp[k]), k
    assert float(e1._rp['g_c2w'].abs().max()) > 0
    if mode == 'render':
        # the fold's inputs come out of the render backward and pp_raygen_select_bwd.  Their float atomics sit in the PARAMETER
        # gradients only; the per-sample and per-ray data gradients have one writer per address, so two runs hand the fold the same
        # bits and it returns the same bits.  On ONE set of inputs it does so whatever came before.
        from poseprobe_amd import ops
        for k in ('go', 'gd', 'gv', 'g_c2w'):
            assert torch.equal(e1._rp[k], e2._rp[k]), k
        ws, r, rows = e1.ws_reproj, e1._rp, rp['rows']
        twice = []
        for _ in range(2):
            out = torch.full_like(r['g_c2w'], float('nan'))
            ops.reproj_pose_fold(e1.cfg.pp, rows['own'], rows['pix'], 192, e1.intr, e1.c2w, e1.w2c, ws.rays_o, ws.rays_d, r['go'],
                                 r['gd'], r['gv'], None, r['g_w2c'], out)
            twice.append(out)
        assert torch.equal(twice[0], twice[1]) and torch.equal(twice[0], r['g_c2w'])


def test_trainer_steps_in_both_modes_without_a_host_copy_in_the_pass():
    """DualBranchTrainer(reprojection=...): a step with two active views (zero-crossing query) and one with three (rendered depth)
    run, move the pose, and leave the scalars on the device."""
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.trainer import DualBranchTrainer
    d = load('reproj_g24.npz')
    opt = bg_nerf.default_options(sample_intvs=16)
    opt.nerf.rand_rays = 48
    eng = _engine(d, reproj_rows=64)
    c = lambda a: torch.tensor(a)
    pairs = [(int(i), int(j), c(d['coord0'][k]), c(d['coord1'][k]), c(d['mconf'][k])) for k, (i, j) in enumerate(zip(d['i_train'], d['j_train']))]
    tr = DualBranchTrainer(eng, opt, max_iter=20, incremental_step=2,
                           reprojection=dict(pairs=pairs, nl=float(d['nl']), weight_projection=1e-3, weight_near_surface=1e-1))
    seen = {}
    for step in range(4):
        before = eng.se3.clone()
        tr.train_step(step)
        assert tr.last_reproj is not None and tr.last_reproj['n_rows'] == 64                # 48 matches -> 32 of them, both directions
        t = eng.last_reproj_terms
        assert all(v.is_cuda for v in t.values())
        seen[tr.last_reproj['mode']] = {k: float(v) for k, v in t.items()}
        assert bool(torch.isfinite(eng.se3).all()) and bool(torch.isfinite(eng.flat.data).all())
        assert not torch.equal(before, eng.se3)
    assert set(seen) == {'crossing', 'render'}
    assert all(v['near'] > 0 and v['n_valid'] > 0 for v in seen.values())
