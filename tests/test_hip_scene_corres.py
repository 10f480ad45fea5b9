"""SPARF correspondence term in the autograd-free scene step: pp_nerf_corres_loss / pp_nerf_pair_pose_bwd against torch
autograd over bg_losses (corres_loss.py:93-222), the union-row pass of DualBranchEngine against an autograd render of the
photometric rays + bg_losses.correspondence_loss, the trainer's loss_type / weight schedules, and a buffer fence around both
kernels."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close, load
from tests.test_hip_step import build_engine

pytestmark = pytest.mark.gpu


def _filters(pixel=False, depth=False, pix_thr=10., dep_thr=0.1):
    from poseprobe_amd import bg_nerf
    return bg_nerf.Options(renderrepro_do_pixel_reprojection_check=pixel, renderrepro_do_depth_reprojection_check=depth,
                           renderrepro_pixel_reprojection_thresh=pix_thr, renderrepro_depth_reprojection_thresh=dep_thr,
                           diff_loss_type='huber')


def _pair_problem(M, seed):
    from poseprobe_amd import synthetic as syn
    H, W = 32, 48
    views = syn.make_views(2, H, W, seed=4)
    w2c = torch.tensor(views['w2c'][:, :3, :4]).float().cuda()
    K = torch.tensor(views['Ks']).float().cuda()
    g = torch.Generator().manual_seed(seed)
    pix_s = (torch.rand(M, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda()
    pix_o = (pix_s.cpu() + torch.randn(M, 2, generator=g) * 3).cuda()
    conf = torch.rand(M, generator=g)
    conf[1::5] = 0.0                                                  # zero-confidence rows still count in the normaliser
    depth = (torch.rand(2, 2 * M, generator=g) * 2.0 + 1.5).cuda()   # [pass][self M | other M]
    return w2c, K, pix_s, pix_o, conf.cuda(), depth


def _torch_corres(opt, w2c, K, pix_s, pix_o, conf, depth, n_pass, weight):
    from poseprobe_amd import bg_losses
    M = pix_s.shape[0]
    bottom = torch.tensor([[0., 0., 0., 1.]], device='cuda')
    T = torch.cat([w2c[1], bottom]) @ bg_losses.pose_inverse_4x4(torch.cat([w2c[0], bottom]))
    total = 0.
    for p in range(n_pass):
        ds, do = depth[p, :M], depth[p, M:]
        total = total + bg_losses.reprojection_loss(opt, pix_s, ds, K[0], pix_o, do, K[1], T, conf[:, None])[0]
        total = total + bg_losses.reprojection_loss(opt, pix_o, do, K[1], pix_s, ds, K[0], bg_losses.pose_inverse_4x4(T),
                                                    conf[:, None])[0]
    return total / (2. * n_pass) * weight


def _cut(v):
    """A threshold between two of the values (never on one: the kernel's and torch's roundings may differ there)."""
    v = v.sort().values
    return float(v[0]) * 2 + 1 if v.numel() == 1 else float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2)


@pytest.mark.parametrize('M', [1, 37, 512, 1500])
@pytest.mark.parametrize('case', ['none', 'pixel', 'depth', 'all_removed'])
def test_corres_kernel_equals_torch_autograd(M, case):
    """Loss, d/d depths and d/d both w2c of pp_nerf_corres_loss == torch autograd through bg_losses.reprojection_loss over both
    directions, one pass (/ 2) and two passes (/ 4)."""
    from poseprobe_amd import bg_losses, ops
    w2c, K, pix_s, pix_o, conf, depth = _pair_problem(M, seed=M)
    weight = 1e-2 / 4
    # thresholds at the median of the unfiltered quantities: about half of the rows pass each filter
    with torch.no_grad():
        bottom = torch.tensor([[0., 0., 0., 1.]], device='cuda')
        T = torch.cat([w2c[1], bottom]) @ bg_losses.pose_inverse_4x4(torch.cat([w2c[0], bottom]))
        proj, z = bg_losses.project_to_other_img(pix_s, depth[0, :M], K[0], K[1], T)
        pix_thr = _cut((proj - pix_o).norm(dim=-1))
        dep_thr = _cut((depth[0, M:] - z).abs() / (depth[0, M:] + 1e-6))
    opt = {'none': _filters(), 'pixel': _filters(pixel=True, pix_thr=pix_thr), 'depth': _filters(depth=True, dep_thr=dep_thr),
           'all_removed': _filters(pixel=True, depth=True, pix_thr=-1.0, dep_thr=dep_thr)}[case]
    for n_pass in (1, 2):
        dep = depth.clone().requires_grad_(True)
        pose = w2c.clone().requires_grad_(True)
        ref = _torch_corres(opt, pose, K, pix_s, pix_o, conf, dep, n_pass, weight)
        ref.backward()
        loss = torch.full((1,), float('nan'), device='cuda')
        g_d = torch.full((2, 2 * M), float('nan'), device='cuda')
        g_w2c = torch.full((2, 3, 4), float('nan'), device='cuda')
        ops.nerf_corres_loss(depth[0], depth[1] if n_pass == 2 else None, pix_s, pix_o, conf, K[0], K[1], w2c[0], w2c[1],
                             opt.renderrepro_do_pixel_reprojection_check, opt.renderrepro_pixel_reprojection_thresh,
                             opt.renderrepro_do_depth_reprojection_check, opt.renderrepro_depth_reprojection_thresh, weight,
                             loss, g_d[0], g_d[1] if n_pass == 2 else None, g_w2c)
        torch.cuda.synchronize()
        what = f'M={M} {case} passes={n_pass}'
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(g_d[:n_pass]).all()) and bool(torch.isfinite(g_w2c).all())
        assert_close(loss[0], ref.detach(), rtol=2e-5, atol=1e-9, name='loss ' + what)
        assert_close(g_d[:n_pass], dep.grad[:n_pass], rtol=1e-4, atol=1e-10, scaled=1e-5, name='g_depth ' + what)
        assert_close(g_w2c, pose.grad, rtol=1e-3, atol=1e-10, scaled=1e-4, name='g_w2c ' + what)
        if case == 'all_removed':
            assert float(loss[0]) == 0.0 and float(g_d[:n_pass].abs().max()) == 0.0 and float(g_w2c.abs().max()) == 0.0
        else:
            assert float(loss[0]) > 0 and float(g_w2c.abs().max()) > 0
            assert bool((g_d[:n_pass].view(n_pass, 2, M)[:, :, 1::5] == 0).all())      # conf = 0 rows get no gradient


def test_pair_pose_fold_equals_torch():
    """pp_nerf_pair_pose_bwd: [sum g_ray (x) dir_cam | sum g_center] of each view's rows + the w2c gradient moved onto c2w
    (camera._PoseChain.backward's algebra), accumulated into the existing g_c2w rows of views i and j only."""
    from poseprobe_amd import camera, ops
    g = torch.Generator().manual_seed(2)
    V, M = 4, 300
    se3 = torch.randn(V, 6, generator=g) * 0.1
    w2c_init = torch.eye(4)[:3].repeat(V, 1, 1)
    w2c_init[:, :, 3] = torch.randn(V, 3, generator=g)
    w2c, c2w = camera.current_pose_c2w(se3.cuda(), w2c_init.cuda(), fix_first=False)
    gc, gr, dc = (torch.randn(2 * M, 3, generator=g).cuda() for _ in range(3))
    g_w2c = torch.randn(2, 3, 4, generator=g).cuda()
    base = torch.randn(V, 3, 4, generator=g).cuda()
    out = base.clone()
    ops.nerf_pair_pose_bwd(gc, gr, dc, w2c.contiguous(), g_w2c, 3, 1, out)
    # reference: autograd of <g_w2c, w2c(c2w)> + the ray / centre algebra w.r.t. c2w
    c = c2w.detach().clone().requires_grad_(True)
    R, t = c[:, :, :3], c[:, :, 3:]
    w2c_of_c = torch.cat([R.transpose(-1, -2), -R.transpose(-1, -2) @ t], dim=-1)
    ray = torch.cat([dc[:M] @ c[3, :, :3].T, dc[M:] @ c[1, :, :3].T])
    cen = torch.cat([c[3, :, 3].expand(M, 3), c[1, :, 3].expand(M, 3)])
    ((ray * gr).sum() + (cen * gc).sum() + (w2c_of_c[3] * g_w2c[0]).sum() + (w2c_of_c[1] * g_w2c[1]).sum()).backward()
    assert_close(out - base, c.grad, rtol=1e-4, atol=1e-5, scaled=1e-5, name='g_c2w')
    assert torch.equal(out[0], base[0]) and torch.equal(out[2], base[2])


def _engines(d, opt, fine, split):
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.joint import DualBranchEngine
    torch.manual_seed(5)
    mk = lambda f: bg_nerf.NeRF(opt, is_fine_network=f, device='cuda', options={'nerf_split': split})
    net, net_f = mk(False), (mk(True) if fine else None)
    for n in (net, net_f):
        if n is not None:
            n.progress.data.fill_(0.6)
            with torch.no_grad():
                n.mlp_feat[-1].bias[0] += 1.0
    eng, _ = build_engine(d)
    return eng, net, net_f, DualBranchEngine(eng, net, depth_range=(0.5, 3.0), scene_net_fine=net_f)


@pytest.mark.parametrize('fine', [False, True])
@pytest.mark.parametrize('split', [1, 0])
def test_joint_step_with_correspondence_term_equals_autograd(fine, split):
    """DualBranchEngine.forward_backward(corres=...) == autograd of se3 -> current_pose_c2w -> SceneRenderer render of the
    photometric rays + 10^-2 / gamma * bg_losses.correspondence_loss on copies of the networks, all draws replayed: L_bg, both
    networks' gradient blocks and the scene share of se3_grad."""
    from poseprobe_amd import bg_losses, bg_nerf, camera
    d = load('forward_g24_s10.npz')
    ray_idx = torch.tensor(d['ray_idx'], dtype=torch.int32, device='cuda')
    jitter = torch.tensor(d['jitter'], device='cuda')
    gs = int(d['global_step'])
    H, W = int(d['H']), int(d['W'])
    opt = bg_nerf.sparf_dtu_options(sample_intvs=24, max_iter=1000)
    opt.nerf.sample_intvs_fine, opt.nerf.fine_sampling = 16, fine
    opt.nerf.ratio_start_fine_sampling_at_x = None
    V, N, S, M, Nf = 3, 40, 24, 29, 16
    g = torch.Generator().manual_seed(3)
    pixels = (torch.rand(N, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda()
    image = torch.rand(V, N, 3, generator=g).cuda()
    rand = torch.rand(V, N, S, 1, generator=g).cuda()
    pix_s = (torch.rand(M, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda()
    pix_o = (pix_s.cpu() + torch.randn(M, 2, generator=g) * 2).cuda()
    conf = torch.rand(M, generator=g).cuda()
    c_rand = torch.rand(2, M, S, 1, generator=g).cuda()
    grid_p, grid_c = torch.rand(Nf + 1, generator=g), torch.rand(Nf + 1, generator=g)
    i, j, weight = 2, 1, 1e-2 / 2

    ref_eng, _ = build_engine(d)                                      # object branch alone
    ref_eng.zero_grads()
    ref_eng.render_and_grads(ray_idx, jitter, gs)
    g_obj = ref_eng.se3_grad.clone()

    eng, net, net_f, joint = _engines(d, opt, fine, split)
    eng.zero_grads()
    _, loss_bg = joint.forward_backward(ray_idx, jitter, gs, pixels, image, depth_rand=rand, fine=fine,
                                        fine_grid=grid_p if fine else None,
                                        corres=dict(i=i, j=j, pix_self=pix_s, pix_other=pix_o, conf=conf, weight=weight),
                                        corres_rand=c_rand, corres_fine_grid=grid_c if fine else None)
    terms = {k: float(v) for k, v in joint.last_scene_terms.items()}
    grads = [st.grad.clone() for st in joint.scene.states]

    # autograd reference on copies of the networks
    se3 = eng.se3.detach().clone().requires_grad_(True)
    w2c, c2w = camera.current_pose_c2w(se3, eng.w2c_init, fix_first=True)
    sr = bg_nerf.SceneRenderer(opt, device='cuda')
    sr.nerf = bg_nerf.NeRF(opt, device='cuda', options={'nerf_split': split})
    sr.nerf.load_state_dict(net.state_dict())
    if fine:
        sr.nerf_fine = bg_nerf.NeRF(opt, is_fine_network=True, device='cuda', options={'nerf_split': split})
        sr.nerf_fine.load_state_dict(net_f.state_dict())
    K = joint.intrinsics()
    pred = sr.render(opt, w2c, H, W, K, pixels=pixels, depth_range=(0.5, 3.0), iter=gs, mode='train', rand=[rand, grid_p])
    photo = bg_nerf.photometric_loss(pred['rgb'], image)
    if fine:
        photo = photo + bg_nerf.photometric_loss(pred['rgb_fine'], image)
    corr, _, rets = bg_losses.correspondence_loss(sr, opt, torch.stack([w2c[i], w2c[j]]), torch.stack([K[i], K[j]]), pix_s, pix_o,
                                                  conf[:, None], H, W, (0.5, 3.0), iteration=gs, rand=[c_rand, grid_c])
    assert ('depth_fine' in rets) == fine
    ref = photo + weight * corr
    ref.backward()
    assert_close(terms['corres'], float(weight * corr.detach()), rtol=1e-4, name='correspondence term')
    assert_close(terms['photometric'], float(photo.detach()), rtol=2e-5, name='photometric term')
    assert_close(loss_bg, ref, rtol=2e-5, name='L_bg')
    assert terms['corres'] > 0
    share = eng.se3_grad - g_obj
    # fine phase: the ray gradients of the hierarchical pass carry the noise test_scene_engine_hierarchical_step_equals_
    # autograd_render allows per ray (assert_mostly_close); their sum over a view meets 1e-2 of the largest entry
    assert_close(share, se3.grad, rtol=1e-3, scaled=1e-2 if fine else 2e-3, name='scene share of the pose gradient')
    # the union pass sums the photometric and matched rows in one pass, the reference in two renders (other row tiles and
    # summation order): the weight-gradient tolerance of test_scene_engine_hierarchical_step_equals_autograd_render
    tol = dict(rtol=1e-3, scaled=1e-2)
    for n_ref, gflat in zip([sr.nerf] + ([sr.nerf_fine] if fine else []), grads):
        for (name, p), gv in zip([(n, p) for n, p in n_ref.named_parameters() if n != 'progress'], n_ref._views(gflat)):
            assert_close(gv, p.grad, name='scene g.' + name, **tol)


def _trainer(d, opt, seed=0, matches=True, **kw):
    from poseprobe_amd.trainer import DualBranchTrainer
    eng, _ = build_engine(d, deterministic_scatter=True)
    eng.zero_grads()
    torch.manual_seed(2)
    sm = None
    if matches:
        g = torch.Generator().manual_seed(11)
        H, W = int(d['H']), int(d['W'])
        sm = []
        for _ in range(3):
            ps = torch.rand(700, 2, generator=g) * torch.tensor([W - 1., H - 1.])
            conf = torch.rand(700, generator=g)
            conf[::4] = 0.0
            sm.append((ps, ps + torch.randn(700, 2, generator=g), conf))
    return DualBranchTrainer(eng, opt, max_iter=10, seed=seed, scene_matches=sm, **kw), eng


def _same_update(a, b, what):
    """Two runs of one step: the networks' weight-gradient GEMMs flush with atomics (pp_gemm_tn_tr.h), and Adam's first step
    g / (|g| + eps) magnifies their rounding where |g| ~ eps - within 1 % of a 1e-3 learning-rate step everywhere, within 1e-7
    on all but 1e-4 of the entries."""
    err = (a - b).abs()
    assert float(err.max()) <= 1e-5 and float((err > 1e-7).float().mean()) <= 1e-4, (what, float(err.max()))


def _step(tr, step):
    torch.manual_seed(100 + step)                                     # the scene sampler draws from the global generators
    return tr.train_step(step)


def test_trainer_depth_cons_adds_nothing_and_no_loss_type_is_unchanged():
    from poseprobe_amd import bg_nerf
    d = load('forward_g24_s10.npz')
    opt = bg_nerf.sparf_dtu_options(sample_intvs=16, max_iter=10)
    opt.nerf.rand_rays = 96
    flats, se3s, terms = [], [], []
    for lt in ('photometric_and_corres_and_depth_cons', 'photometric_and_corres'):
        opt.loss_type = lt
        tr, eng = _trainer(d, opt)
        _step(tr, 0)
        terms.append(tr.last_scene_terms)
        flats.append(tr.nerf.flat.clone())
        se3s.append(eng.se3.clone())
    assert terms[0] is not None and float(terms[0]['corres']) > 0
    assert float(terms[0]['corres']) == float(terms[1]['corres'])                       # bit for bit
    _same_update(flats[0], flats[1], 'scene parameters')
    assert_close(se3s[0], se3s[1], rtol=0, atol=1e-7, name='se3')
    # no loss_type: today's photometric step, whether or not matches are supplied
    base = bg_nerf.default_options(sample_intvs=16)
    base.nerf.rand_rays = 96
    out = []
    for m in (False, True):
        tr, eng = _trainer(d, base, matches=m)
        _step(tr, 0)
        assert tr.last_scene_terms is None and tr.joint.last_scene_terms is None
        out.append((tr.nerf.flat.clone(), eng.se3.clone()))
    _same_update(out[0][0], out[1][0], 'scene parameters without loss_type')
    assert_close(out[0][1], out[1][1], rtol=0, atol=1e-7, name='se3 without loss_type')
    assert not torch.equal(out[0][0], flats[0])                       # the correspondence term did change the update


def test_trainer_gamma_start_iteration_and_active_pairs():
    from poseprobe_amd import bg_nerf
    d = load('forward_g24_s10.npz')
    opt = bg_nerf.sparf_dtu_options(sample_intvs=16, max_iter=10)
    opt.nerf.fine_sampling, opt.nerf.rand_rays = False, 96
    opt.start_iter.corres = 2
    tr, eng = _trainer(d, opt, incremental_step=100)
    k = tr._admit_views(0)
    assert k == 2
    assert tr._corres_batch(1, k) is None                             # before start_iter.corres
    seen = set()
    for _ in range(40):
        c = tr._corres_batch(2, k)
        seen.add((c['i'], c['j']))
        assert c['pix_self'].shape == (48, 2) and c['conf'].shape == (48,) and bool((c['conf'] > 0).all())
    assert seen == {(0, 1), (1, 0)}                                   # only the two active views are paired
    assert tr._corres_batch(4999, k)['weight'] == pytest.approx(1e-2, rel=1e-12)
    assert tr._corres_batch(5000, k)['weight'] == pytest.approx(1e-2 / 2, rel=1e-12)
    for step in range(3):
        _step(tr, step)
        assert (tr.last_scene_terms is None) == (step < 2)
    assert np.isfinite(float(tr.last_scene_terms['corres']))
    # gamma halves the term: the same batch at weight w and w / 2
    c = tr._corres_batch(5000, k)
    pixels, image = torch.rand(20, 2, device='cuda') * 10, torch.rand(2, 20, 3, device='cuda')
    rand, c_rand = torch.rand(2, 20, 16, 1, device='cuda'), torch.rand(2, 48, 16, 1, device='cuda')
    ray_idx = torch.tensor(d['ray_idx'], dtype=torch.int32, device='cuda')
    jitter = torch.tensor(d['jitter'], device='cuda')
    vals = []
    for w in (c['weight'] * 2, c['weight']):
        c['weight'] = w
        tr.joint.forward_backward(ray_idx, jitter, 5000, pixels, image, depth_rand=rand, n_views=2, corres=c, corres_rand=c_rand)
        vals.append(float(tr.joint.last_scene_terms['corres']))
        eng.zero_grads()
        for st in tr.joint.scene.states:
            st.grad.zero_()
    assert vals[0] > 0 and vals[1] == vals[0] / 2


def test_trainer_refuses_unknown_terms_and_sharded_correspondences():
    from poseprobe_amd import bg_nerf
    d = load('forward_g24_s10.npz')
    opt = bg_nerf.sparf_dtu_options(sample_intvs=16, max_iter=10)
    opt.nerf.rand_rays = 96
    opt.loss_type = 'photometric_and_SparseCOLMAPDepthLoss'
    with pytest.raises(NotImplementedError):
        _trainer(d, opt)
    opt.loss_type = 'photometric_and_corres'
    tr, eng = _trainer(d, opt)
    c = tr._corres_batch(0, 3)
    eng.dist = object()                                               # any distributed context
    try:
        with pytest.raises(NotImplementedError):
            tr.joint.forward_backward(None, None, 0, None, None, corres=c)
    finally:
        eng.dist = None


def test_corres_kernels_stay_inside_their_buffers():
    """Both kernels write only inside their outputs: every caller-owned buffer they write sits in a 64 KB-sentineled arena, at
    M = 1, 512 (the reference's cap) and 1500 (several rows per thread).  Run once per case, no repetition."""
    from poseprobe_amd import ops
    PAD, SENT = 16384, 0x7FC0DEAD

    def fenced(n):
        arena = torch.empty(n + 2 * PAD, dtype=torch.int32, device='cuda').fill_(SENT).view(torch.float32)
        return arena, arena[PAD:PAD + n]

    def intact(arena, n, what):
        a = arena.view(torch.int32)
        assert bool((a[:PAD] == SENT).all()) and bool((a[PAD + n:] == SENT).all()), what

    for M in (1, 512, 1500):
        w2c, K, pix_s, pix_o, conf, depth = _pair_problem(M, seed=7)
        la, loss = fenced(1)
        d0a, gd0 = fenced(2 * M)
        d1a, gd1 = fenced(2 * M)
        wa, g_w2c = fenced(24)
        ops.nerf_corres_loss(depth[0], depth[1], pix_s, pix_o, conf, K[0], K[1], w2c[0], w2c[1], True, 30.0, True, 0.5, 0.01,
                             loss, gd0, gd1, g_w2c)
        torch.cuda.synchronize()
        for arena, n, what in ((la, 1, 'loss'), (d0a, 2 * M, 'g_depth0'), (d1a, 2 * M, 'g_depth1'), (wa, 24, 'g_w2c')):
            intact(arena, n, f'corres M={M} {what}')
        V = 3
        ca, g_c2w = fenced(V * 12)
        g_c2w.zero_()
        g = torch.Generator().manual_seed(M)
        gc, gr, dc = (torch.randn(2 * M, 3, generator=g).cuda() for _ in range(3))
        w2cV = torch.cat([w2c, w2c[:1]]).contiguous()
        ops.nerf_pair_pose_bwd(gc, gr, dc, w2cV, g_w2c.view(2, 3, 4), 2, 0, g_c2w.view(V, 3, 4))
        torch.cuda.synchronize()
        intact(ca, V * 12, f'pair pose M={M} g_c2w')
        assert float(g_c2w[12:24].abs().max()) == 0.0 and float(g_c2w.abs().max()) > 0
