"""GPU tests of the scene branch's deterministic mode: bg_nerf.SceneEngine(deterministic=True) and
joint.DualBranchEngine(deterministic=True).  The ordered flush of the weight-gradient kernel (csrc/pp_gemm_tn_tr.h),
the sampler kernel of the fine phase and the pose fold make the scene step and the whole joint step bit-reproducible; with the
keyword off nothing changes."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close, load
from tests.test_hip_deterministic import ORDER_TOL, assert_same_bits, snapshot
from tests.test_hip_step import build_engine

pytestmark = pytest.mark.gpu

NF = 16                     # fine samples of the small problems


def _opt(S, fine=True):
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.sparf_dtu_options(sample_intvs=S, max_iter=1000)
    opt.nerf.sample_intvs_fine, opt.nerf.fine_sampling = NF, fine
    opt.nerf.ratio_start_fine_sampling_at_x = None
    return opt


def _nets(opt, seed=5, d=None, options=None):
    """Coarse and fine network: seeded initialisation (the fixture's parameters in the coarse one when `d` is given), density
    bias raised so that the rays are not empty."""
    from poseprobe_amd import bg_nerf
    torch.manual_seed(seed)
    nets = [bg_nerf.NeRF(opt, is_fine_network=f, device='cuda', options=options) for f in (False, True)]
    for n in nets:
        n.progress.data.fill_(0.6)
        with torch.no_grad():
            n.mlp_feat[-1].bias[0] += 1.0
    if d is not None:
        sd = {k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('param.')}
        sd['progress'] = torch.tensor(float(d['progress']))
        nets[0].load_state_dict(sd)
    return nets


def scene_state(eng):
    out = {}
    for i, st in enumerate(eng.states):
        out.update({f'net{i}.flat': st.net.flat, f'net{i}.m': st.m, f'net{i}.v': st.v})
    return out


def scene_snapshot(eng, extra=()):
    torch.cuda.synchronize()
    out = {k: v.detach().clone() for k, v in scene_state(eng).items()}
    out.update({k: v.detach().clone() for k, v in extra})
    return out


def assert_same_scene_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} entries'


# ------------------------------------------------------------------------------------------------ 1. scene engine alone
def scene_problem(shape):
    """scene_b2.npz's rays (48 x 16 samples), or the reference batch 1023 x 128 (every row split of the weight-gradient kernel
    active, a ragged last one) from a seeded generator."""
    g = torch.Generator().manual_seed(17)
    if shape == 'fixture':
        d = load('scene_b2.npz')
        R, S = int(d['B']) * int(d['N']), int(d['S'])
        center, ray = torch.tensor(d['center']).reshape(R, 3), torch.tensor(d['ray']).reshape(R, 3)
        depth = torch.tensor(d['depth_samples']).reshape(R, S)
        image = torch.tensor(d['loss_image']).reshape(R, 3)
        lo, hi = float(depth.min()) - 1e-3, float(depth.max()) + 1e-3
    else:
        d, (R, S) = None, shape
        center, ray = torch.randn(R, 3, generator=g) * 0.3, torch.randn(R, 3, generator=g)
        lo, hi = 0.4, 2.4
        depth = (torch.rand(R, S, generator=g) + torch.arange(S)) / S * (hi - lo) + lo
        image = torch.rand(R, 3, generator=g)
    grids = [torch.rand(NF + 1, generator=g) for _ in range(5)]
    return d, S, [t.cuda().contiguous() for t in (center, ray, depth, image)], (lo, hi), grids


def run_scene(shape, fine, n_steps=5, **kw):
    from poseprobe_amd import bg_nerf
    d, S, (center, ray, depth, image), rng, grids = scene_problem(shape)
    net, net_f = _nets(_opt(S), d=d)
    eng = bg_nerf.SceneEngine(net, lr=1e-3, net_fine=net_f, **kw)
    out = []
    for s in range(n_steps):
        loss, gc, gr = eng.step(center, ray, depth, image, fine=fine, depth_range=rng, fine_grid=grids[s])
        out.append(scene_snapshot(eng, (('g_center', gc), ('g_ray', gr))))
    return eng, out


@pytest.mark.parametrize('fine', [False, True])
@pytest.mark.parametrize('shape', ['fixture', (1023, 128)])
def test_scene_engine_trajectory_is_bit_reproducible(shape, fine):
    """Two separately built deterministic SceneEngines, five steps with replayed draws: flat, m, v of both networks and the
    returned ray gradients equal bit for bit after every step."""
    ea, a = run_scene(shape, fine, deterministic=True)
    eb, b = run_scene(shape, fine, deterministic=True)
    assert ea._ordered_work is not None and ea._ordered_work.data_ptr() != eb._ordered_work.data_ptr()
    assert bool((a[-1]['net0.flat'] != a[0]['net0.flat']).any())
    assert bool((a[-1]['net1.flat'] != a[0]['net1.flat']).any()) == fine
    for s, (x, y) in enumerate(zip(a, b)):
        assert_same_scene_bits(x, y, f'{shape} fine={fine} step {s + 1}')


# ------------------------------------------------------------------------------------------------ 2. joint step
def joint_problem():
    """Object branch: forward_g24_s10.npz.  Scene branch: 3 views x 40 pixels x 24 samples; the matched rows are
    scene_corres.npz's (64 pairs)."""
    d = load('forward_g24_s10.npz')
    c = load('scene_corres.npz')
    H, W = int(d['H']), int(d['W'])
    V, N, S, M = 3, 40, 24, int(c['N'])
    g = torch.Generator().manual_seed(3)
    P = dict(d=d, V=V, N=N, S=S, M=M,
             pixels=(torch.rand(N, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda(),
             image=torch.rand(V, N, 3, generator=g).cuda(),
             pix_s=torch.tensor(c['pix_self']).float().cuda().contiguous(), pix_o=torch.tensor(c['pix_other']).float().cuda().contiguous(),
             conf=torch.tensor(c['conf']).float().reshape(-1).cuda())
    P['draws'] = [dict(rand=torch.rand(V, N, S, 1, generator=g).cuda(), c_rand=torch.rand(2, M, S, 1, generator=g).cuda(),
                       grid_p=torch.rand(NF + 1, generator=g), grid_c=torch.rand(NF + 1, generator=g)) for _ in range(5)]
    return P


def build_joint(P, deterministic, options=None):
    from poseprobe_amd.joint import DualBranchEngine
    net, net_f = _nets(_opt(P['S']), options=options)
    eng, _ = build_engine(P['d'], pose_iters=1000, deterministic=deterministic)
    eng.zero_grads()
    return DualBranchEngine(eng, net, depth_range=(0.5, 3.0), scene_net_fine=net_f, deterministic=deterministic)


def joint_kwargs(P, s, fine, corres):
    dr = P['draws'][s]
    kw = dict(depth_rand=dr['rand'], fine=fine, fine_grid=dr['grid_p'] if fine else None)
    if corres:
        kw.update(corres=dict(i=2, j=1, pix_self=P['pix_s'], pix_other=P['pix_o'], conf=P['conf'], weight=1e-2 / 2),
                  corres_rand=dr['c_rand'], corres_fine_grid=dr['grid_c'] if fine else None)
    return kw


def run_joint(P, fine, corres, n_steps=5, deterministic=True):
    """-> per-step snapshots (object state, scene state) of a free-running joint trajectory."""
    from poseprobe_amd import synthetic as syn
    joint = build_joint(P, deterministic)
    d = P['d']
    V, H, W = d['images'].shape[:3]
    out = []
    for s in range(n_steps):
        idx, jit = syn.step_randomness(V * H * W, int(d['n_rand']), seed=40 + s)
        idx, jit = torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda')
        kw = joint_kwargs(P, s, fine, corres)
        # (train_step takes no replayed correspondence draws: forward_backward + the two optimiser steps it runs on one GPU)
        joint.forward_backward(idx, jit, 10 + s, P['pixels'], P['image'], **kw)
        joint.obj.optimizer_step(True, grad_scale=1.0)
        joint.scene.optimizer_step()
        out.append((snapshot(joint.obj), scene_snapshot(joint.scene)))
    return out


@pytest.mark.parametrize('fine,corres', [(False, False), (True, False), (False, True), (True, True)])
def test_joint_trajectory_is_bit_reproducible(fine, corres):
    """Two separately built deterministic DualBranchEngines, five free-running joint steps on the same draws: all nine object
    tensors and flat, m, v of both scene networks equal bit for bit after every step."""
    P = joint_problem()
    a, b = run_joint(P, fine, corres), run_joint(P, fine, corres)
    assert bool((a[-1][0]['se3'] != a[0][0]['se3']).any()) and bool((a[-1][1]['net0.flat'] != a[0][1]['net0.flat']).any())
    for s, ((oa, sa), (ob, sb)) in enumerate(zip(a, b)):
        what = f'fine={fine} corres={corres} step {s + 1}'
        assert_same_bits(oa, ob, what)
        assert_same_scene_bits(sa, sb, what)


# ------------------------------------------------------------------------------------------------ 3. same gradients as the default
def test_deterministic_joint_pass_computes_the_same_gradients_as_the_default_one():
    """One forward_backward (coarse phase + correspondence rows: there only the summation order differs - the fine phase also
    draws its samples with another kernel) from the same state: every scene parameter gradient and se3_grad within ORDER_TOL of the
    default engine's."""
    from poseprobe_amd import synthetic as syn
    P = joint_problem()
    d = P['d']
    V, H, W = d['images'].shape[:3]
    idx, jit = syn.step_randomness(V * H * W, int(d['n_rand']), seed=91)
    idx, jit = torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda')
    res = []
    for det in (False, True):
        joint = build_joint(P, det)
        joint.forward_backward(idx, jit, 10, P['pixels'], P['image'], **joint_kwargs(P, 0, False, True))
        torch.cuda.synchronize()
        res.append((joint.scene.states[0].grad.clone(), joint.obj.se3_grad.clone()))
        assert (joint.scene._ordered_work is not None) == det
    (g0, s0), (g1, s1) = res
    assert float(g0.abs().max()) > 0 and float(s0.abs().max()) > 0
    net = _nets(_opt(P['S']))[0]
    for (name, _), a, b in zip([(n, p) for n, p in net.named_parameters() if n != 'progress'], net._views(g1), net._views(g0)):
        print(f'deterministic vs default g.{name}: max |diff| {float((a - b).abs().max()):.3e}, max |ref| {float(b.abs().max()):.3e}')
        assert_close(a, b, name=f'deterministic vs default: scene g.{name}', **ORDER_TOL)
    print(f'deterministic vs default se3_grad: max |diff| {float((s1 - s0).abs().max()):.3e}, max |ref| {float(s0.abs().max()):.3e}')
    assert_close(s1, s0, name='deterministic vs default: se3_grad', **ORDER_TOL)


# ------------------------------------------------------------------------------------------------ 4. parity at the default thresholds
def test_scene_fixture_parity_with_the_ordered_flush():
    """tests/test_hip_scene.py::test_scene_matches_reference_outputs_and_backward with the network of a deterministic engine (its
    context carries the workspace, so the backward pass below flushes in order): same thresholds."""
    from poseprobe_amd import bg_nerf
    d = load('scene_b2.npz')
    opt = bg_nerf.default_options()
    net = bg_nerf.NeRF(opt, device='cuda')
    sd = {k[6:]: torch.tensor(v) for k, v in d.items() if k.startswith('param.')}
    sd['progress'] = torch.tensor(float(d['progress']))
    net.load_state_dict(sd)
    eng = bg_nerf.SceneEngine(net, deterministic=True)
    assert net.ctx is not None and eng._ordered_work is not None
    center = torch.tensor(d['center']).cuda().requires_grad_(True)
    ray = torch.tensor(d['ray']).cuda().requires_grad_(True)
    depth = torch.tensor(d['depth_samples']).cuda()
    pred = net.composite(opt, ray, net.forward_samples(opt, center, ray, depth, mode='train'), depth)
    for k in ('rgb_samples', 'density_samples', 'rgb', 'rgb_var', 'depth', 'depth_var', 'opacity', 'weights', 'all_cumulated'):
        assert_close(pred[k], d['out.' + k], rtol=2e-5, atol=2e-6, name=k)
    total = 0.
    for k in ('rgb', 'depth', 'opacity', 'weights', 'rgb_samples', 'density_samples'):
        total = total + (torch.tensor(d['lf_coef_' + k]).cuda() * pred[k]).sum()
    assert_close(total, d['lf_value'], rtol=1e-5, atol=1e-4, name='lf_value')
    total.backward()
    assert_close(center.grad, d['lf_g_center'], rtol=1e-4, scaled=2e-5, name='g_center')
    assert_close(ray.grad, d['lf_g_ray'], rtol=1e-4, scaled=2e-5, name='g_ray')
    for name, p in net.named_parameters():
        if name != 'progress':
            assert_close(p.grad, d['lf_g.' + name], rtol=1e-4, scaled=2e-5, name='g.' + name)
    # the engine's own pass on the fixture's photometric problem: the reference's render loss
    R, S = int(d['B']) * int(d['N']), int(d['S'])
    loss, _, _ = eng.forward_backward(center.detach().reshape(R, 3), ray.detach().reshape(R, 3), depth.reshape(R, S).contiguous(),
                                      torch.tensor(d['loss_image']).cuda().reshape(R, 3))
    assert_close(loss, d['loss_render'], rtol=2e-5, name='loss_render')


@pytest.mark.parametrize('fine', [False, True])
def test_deterministic_joint_step_with_correspondence_rows_equals_autograd(fine):
    """tests/test_hip_scene_corres.py::test_joint_step_with_correspondence_term_equals_autograd with deterministic engines and
    scene_corres.npz's matched rows: same thresholds."""
    from poseprobe_amd import bg_losses, bg_nerf, camera
    P = joint_problem()
    d = P['d']
    ray_idx = torch.tensor(d['ray_idx'], dtype=torch.int32, device='cuda')
    jitter = torch.tensor(d['jitter'], device='cuda')
    gs, H, W = int(d['global_step']), int(d['H']), int(d['W'])
    i, j, weight = 2, 1, 1e-2 / 2
    dr = P['draws'][0]
    ref_eng, _ = build_engine(d, deterministic=True)                  # object branch alone
    ref_eng.zero_grads()
    ref_eng.render_and_grads(ray_idx, jitter, gs)
    g_obj = ref_eng.se3_grad.clone()

    opt = _opt(P['S'], fine)
    torch.manual_seed(5)
    net = bg_nerf.NeRF(opt, device='cuda')
    net_f = bg_nerf.NeRF(opt, is_fine_network=True, device='cuda') if fine else None
    for n in (net, net_f):
        if n is not None:
            n.progress.data.fill_(0.6)
            with torch.no_grad():
                n.mlp_feat[-1].bias[0] += 1.0
    from poseprobe_amd.joint import DualBranchEngine
    eng, _ = build_engine(d, deterministic=True)
    joint = DualBranchEngine(eng, net, depth_range=(0.5, 3.0), scene_net_fine=net_f, deterministic=True)
    eng.zero_grads()
    _, loss_bg = joint.forward_backward(ray_idx, jitter, gs, P['pixels'], P['image'], **joint_kwargs(P, 0, fine, True))
    terms = {k: float(v) for k, v in joint.last_scene_terms.items()}
    grads = [st.grad.clone() for st in joint.scene.states]

    se3 = eng.se3.detach().clone().requires_grad_(True)
    w2c, c2w = camera.current_pose_c2w(se3, eng.w2c_init, fix_first=True)
    sr = bg_nerf.SceneRenderer(opt, device='cuda')
    sr.nerf = bg_nerf.NeRF(opt, device='cuda')
    sr.nerf.load_state_dict(net.state_dict())
    if fine:
        sr.nerf_fine = bg_nerf.NeRF(opt, is_fine_network=True, device='cuda')
        sr.nerf_fine.load_state_dict(net_f.state_dict())
    K = joint.intrinsics()
    pred = sr.render(opt, w2c, H, W, K, pixels=P['pixels'], depth_range=(0.5, 3.0), iter=gs, mode='train', rand=[dr['rand'], dr['grid_p']])
    photo = bg_nerf.photometric_loss(pred['rgb'], P['image'])
    if fine:
        photo = photo + bg_nerf.photometric_loss(pred['rgb_fine'], P['image'])
    corr, _, rets = bg_losses.correspondence_loss(sr, opt, torch.stack([w2c[i], w2c[j]]), torch.stack([K[i], K[j]]), P['pix_s'], P['pix_o'],
                                                  P['conf'][:, None], H, W, (0.5, 3.0), iteration=gs, rand=[dr['c_rand'], dr['grid_c']])
    assert ('depth_fine' in rets) == fine
    ref = photo + weight * corr
    ref.backward()
    assert_close(terms['corres'], float(weight * corr.detach()), rtol=1e-4, name='correspondence term')
    assert_close(terms['photometric'], float(photo.detach()), rtol=2e-5, name='photometric term')
    assert_close(loss_bg, ref, rtol=2e-5, name='L_bg')
    assert terms['corres'] > 0
    assert_close(eng.se3_grad - g_obj, se3.grad, rtol=1e-3, scaled=1e-2 if fine else 2e-3, name='scene share of the pose gradient')
    for n_ref, gflat in zip([sr.nerf] + ([sr.nerf_fine] if fine else []), grads):
        for (name, p), gv in zip([(n, p) for n, p in n_ref.named_parameters() if n != 'progress'], n_ref._views(gflat)):
            assert_close(gv, p.grad, name='scene g.' + name, rtol=1e-3, scaled=1e-2)


# ------------------------------------------------------------------------------------------------ 5. ragged size, canaries
def test_deterministic_pass_stays_inside_its_buffers_at_a_ragged_size():
    """One deterministic backward at 37 x 50 = 1850 rows (no multiple of 64; 29 of the 85 .. 256 row splits of a product get rows,
    the others return before the flush) with 64 KB of canary words in front of and behind the workspace and the gradient block:
    the canaries are intact, the gradients within ORDER_TOL of the default path's.  Run once, as the other fences."""
    from poseprobe_amd import bg_nerf, ops
    PAD, SENT = 16384, 0x7FC0DEAD

    def fenced(n_floats, fill=None):
        arena = torch.empty(n_floats + 2 * PAD, dtype=torch.int32, device='cuda').fill_(SENT).view(torch.float32)
        body = arena[PAD:PAD + n_floats]
        if fill is not None:
            body.fill_(fill)
        return arena, body

    def intact(arena, n, what):
        a = arena.view(torch.int32)
        assert bool((a[:PAD] == SENT).all()), f'{what}: canaries IN FRONT of the buffer were overwritten'
        assert bool((a[PAD + n:] == SENT).all()), f'{what}: canaries BEHIND the buffer were overwritten'

    R, S = 37, 50
    M = R * S
    assert M % 64 != 0
    opt = bg_nerf.default_options(sample_intvs=S)
    torch.manual_seed(3)
    net = bg_nerf.NeRF(opt, device='cuda', options={'nerf_split': 1})
    net.progress.data.fill_(0.7)
    g = torch.Generator().manual_seed(21)
    center, ray = (torch.randn(R, 3, generator=g) * 0.3).cuda(), torch.randn(R, 3, generator=g).cuda()
    depth = ((torch.rand(R, S, generator=g) + torch.arange(S)) / S * 2.0 + 0.4).cuda().contiguous()
    g_rgb, g_den = torch.randn(M, 3, generator=g).cuda(), torch.randn(M, generator=g).cuda()
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    n_acts, n_scr = ops.nerf_workspace(M, R)
    acts, scr = torch.empty(n_acts, device='cuda'), torch.zeros(n_scr, device='cuda')
    rgb_s, dens = torch.empty(M, 3, device='cuda'), torch.empty(M, device='cuda')
    ops.nerf_fwd(net.flat, center, ray, depth, net.band_weights(), count, R, S, acts, rgb_s, dens, net.ctx)
    gc, gr = torch.empty(R, 3, device='cuda'), torch.empty(R, 3, device='cuda')
    ref = torch.zeros_like(net.flat)
    ops.nerf_bwd(net.flat, ray, depth, count, R, S, acts, rgb_s, g_rgb, g_den, scr, ref, gc, gr, net.ctx)
    torch.cuda.synchronize()
    n_work = ops.nerf_ordered_workspace() // 4
    work_a, work = fenced(n_work)
    pg_a, pgrad = fenced(net.flat.numel(), 0.0)
    ops.nerf_ordered_attach(net.ctx, work.view(torch.uint8))
    ops.nerf_bwd(net.flat, ray, depth, count, R, S, acts, rgb_s, g_rgb, g_den, scr, pgrad, gc, gr, net.ctx)
    torch.cuda.synchronize()
    ops.nerf_ordered_attach(net.ctx, None)
    intact(work_a, n_work, 'workspace')
    intact(pg_a, net.flat.numel(), 'params_grad')
    assert bool(torch.isfinite(pgrad).all()) and float(ref.abs().max()) > 0
    print(f'ragged pass: max |diff| {float((pgrad - ref).abs().max()):.3e}, max |ref| {float(ref.abs().max()):.3e}')
    for (name, _), a, b in zip([(n, p) for n, p in net.named_parameters() if n != 'progress'], net._views(pgrad), net._views(ref)):
        assert_close(a, b, name=f'ordered vs atomic flush: g.{name}', **ORDER_TOL)


def test_layer_by_layer_backward_with_the_ordered_flush_repeats_its_bits():
    """The layer-by-layer backward (nerf_chain = 0) at 37 x 50 (ragged last tile) with an ordered-flush workspace attached: its nine
    weight-gradient products run back to back, behind the data gradients, through the one set of ordered slots.  Two calls on
    the same inputs give the same bits in params_grad, g_center and g_ray; against the fused route on the same forward state (the
    fused forward's activation block, mask planes re-packed) they agree within the tolerances of
    tests/test_hip_scene.py::test_scene_trunk_kernel_equals_layer_by_layer_path."""
    from poseprobe_amd import bg_nerf, ops
    from tests.test_hip_scene import repack_masks_for_the_layer_by_layer_backward
    R, S = 37, 50
    M = R * S
    opt = bg_nerf.default_options(sample_intvs=S)
    torch.manual_seed(3)
    fused, layered = (bg_nerf.NeRF(opt, device='cuda', options={'nerf_chain': c}) for c in (3, 0))
    with torch.no_grad():
        layered.flat.copy_(fused.flat)
    for n in (fused, layered):
        n.progress.data.fill_(0.7)
    g = torch.Generator().manual_seed(23)
    center, ray = (torch.randn(R, 3, generator=g) * 0.3).cuda(), torch.randn(R, 3, generator=g).cuda()
    depth = ((torch.rand(R, S, generator=g) + torch.arange(S)) / S * 2.0 + 0.4).cuda().contiguous()
    g_rgb, g_den = torch.randn(M, 3, generator=g).cuda(), torch.randn(M, generator=g).cuda()
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    n_acts, n_scr = ops.nerf_workspace(M, R)
    acts = torch.zeros(n_acts, device='cuda')
    rgb_s, dens = torch.empty(M, 3, device='cuda'), torch.empty(M, device='cuda')
    ops.nerf_fwd(fused.flat, center, ray, depth, fused.band_weights(), count, R, S, acts, rgb_s, dens, fused.ctx)
    acts_l = repack_masks_for_the_layer_by_layer_backward(acts, M)

    def backward(net, a):
        pg = torch.zeros_like(net.flat)
        gc, gr = torch.full((R, 3), float('nan'), device='cuda'), torch.full((R, 3), float('nan'), device='cuda')
        ops.nerf_bwd(net.flat, ray, depth, count, R, S, a, rgb_s, g_rgb, g_den, torch.zeros(n_scr, device='cuda'), pg, gc, gr, net.ctx)
        torch.cuda.synchronize()
        return pg, gc, gr

    ref = backward(fused, acts)
    work = torch.empty(ops.nerf_ordered_workspace(), dtype=torch.uint8, device='cuda')
    ops.nerf_ordered_attach(layered.ctx, work)
    one, two = backward(layered, acts_l), backward(layered, acts_l)
    ops.nerf_ordered_attach(layered.ctx, None)
    assert float(one[0].abs().max()) > 0
    for name, a, b, r in zip(('params_grad', 'g_center', 'g_ray'), one, two, ref):
        assert bool(torch.isfinite(a).all())
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{name}: two calls differ in {int((a != b).sum())} of {a.numel()} entries'
        print(f'layer-by-layer (ordered) vs fused {name}: max |diff| {float((a - r).abs().max()):.3e}, max |ref| {float(r.abs().max()):.3e}')
        assert_close(a, r, rtol=2e-5, scaled=2e-5, name=f'layer-by-layer (ordered) vs fused: {name}')


# ------------------------------------------------------------------------------------------------ 6. pose fold
def fold_inputs(V=3, N=1024, seed=7):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(V, N, 3, generator=g) for _ in range(3))          # g_ray, g_center, dir_cam


def fold_expression(g_ray, g_center, dir_cam):
    """joint.DualBranchEngine's fold, in the dtype of its inputs."""
    return torch.cat([torch.einsum('vni,vnj->vij', g_ray, dir_cam), g_center.sum(1)[..., None]], dim=-1)


# Error of the fp32 torch expression (CPU) against its float64 evaluation on fold_inputs(): 4.97e-7 of the largest entry (V = 3,
# N = 1024; tests/test_scene_deterministic_host.py re-measures it).  The kernel is another summation order of the same length: it
# is allowed 4 x that.
FOLD_FP32_ERR = 5.0e-7
FOLD_TOL = 4 * FOLD_FP32_ERR


def test_c2w_fold_kernel_equals_the_float64_expression():
    from poseprobe_amd import ops
    g_ray, g_center, dir_cam = fold_inputs()
    ref = fold_expression(g_ray.double(), g_center.double(), dir_cam.double())
    out = torch.full((5, 3, 4), float('nan'), device='cuda')
    ops.nerf_c2w_fold(g_ray.cuda(), g_center.cuda(), dir_cam.cuda(), out)
    torch.cuda.synchronize()
    err = float((out[:3].cpu().double() - ref).abs().max() / ref.abs().max())
    print(f'pp_nerf_c2w_fold: error {err:.3e} of the largest entry (allowed {FOLD_TOL:.1e})')
    assert err <= FOLD_TOL
    assert float(out[3:].abs().max()) == 0.0                          # views that are not in play


# ------------------------------------------------------------------------------------------------ 7. sampler
def pdf_inputs(R=96, S=128, Nf=128, per_ray=False, det=False, seed=9):
    """Strictly positive, smooth weights (softmax of a low-frequency signal): no degenerate bin.  -> weights, coarse depths
    [R, S], grid [Nf + 1] or [R, Nf + 1], depth range."""
    g = torch.Generator().manual_seed(seed + 2 * per_ray + det)
    lo, hi = 0.5, 3.0
    x = torch.linspace(0, 1, S)[None]
    sig = sum(torch.randn(R, 1, generator=g) * torch.sin((k + 1) * 3.1 * x + 6.3 * torch.rand(R, 1, generator=g)) for k in range(3))
    w = torch.softmax(0.4 * sig, dim=-1) * (0.3 + 0.7 * torch.rand(R, 1, generator=g))
    depth = (torch.rand(R, S, generator=g) + torch.arange(S)) / S * (hi - lo) + lo
    if det:
        grid = torch.linspace(0, 1, Nf + 1)
        grid = grid.expand(R, Nf + 1).contiguous() if per_ray else grid
    else:
        grid = torch.rand(R, Nf + 1, generator=g) if per_ray else torch.rand(Nf + 1, generator=g)
    return w.contiguous(), depth.contiguous(), grid, (lo, hi)


def pdf_expression(w, depth, grid, rng, Nf):
    """bg_nerf.sample_depth_from_pdf + the merge of SceneEngine.forward_backward, in the dtype of the inputs."""
    from poseprobe_amd import bg_nerf
    S = w.shape[1]
    fine_t = bg_nerf.sample_depth_from_pdf(w[None], S, Nf, rng, det=False, grid=grid)
    return torch.cat([depth, fine_t[0, :, :, 0].to(depth.dtype)], dim=1).sort(dim=1).values


# Error of the fp32 torch expression (CPU) against its float64 evaluation in the four cases below, in depth units (range 0.5 .. 3):
# 8.2e-7 (shared, det), 1.09e-6 (shared, random), 1.07e-6 (per ray, det), 1.43e-6 (per ray, random); the host test file re-measures
# them.  The kernel is allowed 4 x the largest.
PDF_FP32_ERR = 1.43e-6
PDF_TOL = 4 * PDF_FP32_ERR


@pytest.mark.parametrize('per_ray', [False, True])
@pytest.mark.parametrize('det', [True, False])
def test_sample_pdf_kernel_equals_the_float64_expression(per_ray, det):
    from poseprobe_amd import ops
    Nf = 128
    w, depth, grid, rng = pdf_inputs(per_ray=per_ray, det=det)
    ref = pdf_expression(w.double(), depth.double(), grid.double(), rng, Nf)
    out = torch.full((w.shape[0], w.shape[1] + Nf), float('nan'), device='cuda')
    ops.nerf_sample_pdf(w.cuda(), depth.cuda(), grid.cuda(), Nf, rng, out)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[:, 1:] >= got[:, :-1]).all())
    err = float((got.double() - ref).abs().max())
    print(f'pp_nerf_sample_pdf per_ray={per_ray} det={det}: max error {err:.3e} (allowed {PDF_TOL:.1e})')
    assert err <= PDF_TOL


# ------------------------------------------------------------------------------------------------ 8. keyword off / refusals
def test_keyword_off_is_the_default_path_and_the_fp32_instruction_path_is_refused():
    from poseprobe_amd import _lib, bg_nerf, ops
    opt = _opt(16)
    net, net_f = _nets(opt)
    before = torch.cuda.memory_allocated()
    eng = bg_nerf.SceneEngine(net, net_fine=net_f, deterministic=False)
    grown = torch.cuda.memory_allocated() - before
    assert net.ctx is None and net_f.ctx is None and eng._ordered_work is None and not eng.deterministic
    assert grown < ops.nerf_ordered_workspace() - 2 ** 22              # gradient blocks and moments (14 MB), not the 32 MB workspace
    with pytest.raises(ValueError, match='deterministic=True with nerf_split = 0'):
        bg_nerf.SceneEngine(_nets(opt, options={'nerf_split': 0})[0], deterministic=True)
    # the library itself refuses, too: a workspace attached to a context whose options select the fp32-instruction kernel
    ctx = ops.Context(nerf_split=0)
    work = torch.empty(ops.nerf_ordered_workspace(), dtype=torch.uint8, device='cuda')
    ops.nerf_ordered_attach(ctx, work)
    R, S = 4, 8
    M = R * S
    n_acts, n_scr = ops.nerf_workspace(M, R)
    z = lambda *s: torch.zeros(*s, device='cuda')
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    with pytest.raises(_lib.PoseProbeError, match='ordered'):
        ops.nerf_bwd(net.flat, z(R, 3), z(R, S), count, R, S, z(n_acts), z(M, 3), z(M, 3), z(M), z(n_scr), torch.zeros_like(net.flat),
                     z(R, 3), z(R, 3), ctx)
