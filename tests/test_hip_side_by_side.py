"""Launches that carry independent small kernels as work-group roles beside a neighbour: the optimiser tail beside
the grid pass, the colour lookup beside the geometry forward.

Every test runs the SEPARATE launches and the fused launch from one saved state and compares the two.  Every role runs the code
of its stand-alone kernel on the same inputs, so whatever is not a float atomic sum has to be bit-identical.  The atomic sums
(tv_out; c2w_grad and the se3 quantities that follow from it) are the same terms added in another order; their bounds are written
where they are used and are the ones the existing tests of those kernels use against their references
(optim_cases.TOL['grid.tv'], 64 float32 ulps of the largest entry of a view's c2w_grad in test_hip_stage_kernels).
"""
import numpy as np
import pytest
import torch

from tests import optim_cases as K
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
XYZ_MIN = np.array([-0.6, -0.55, -0.7], np.float32)
XYZ_MAX = np.array([0.6, 0.5, 0.45], np.float32)
ADAM = (K.B1, K.B2, K.EPS)
POSE_ADAM = (0.9, 0.999, 1e-8)


def same_bits(a, b, what):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape, f'{what}: shapes {tuple(a.shape)} {tuple(b.shape)}'
    same = (a == b) | (torch.isnan(a) & torch.isnan(b)) if a.is_floating_point() else (a == b)
    assert bool(same.all()), f'{what}: {int((~same).sum())} of {a.numel()} entries differ'


def scene(world_size):
    from poseprobe_amd import ops
    vox = float(np.prod(XYZ_MAX - XYZ_MIN) / np.prod(world_size)) ** (1 / 3)
    return ops.make_scene(XYZ_MIN, XYZ_MAX, world_size, vox, 0.5, 0.24, 4.8, 0.0, k0_dim=12, pos_pe=5, view_pe=1)


# ------------------------------------------------------------------------------------------------------------ grid + tail
GRID_SHAPES = [(5, 4, 3, 12), (9, 10, 7, 12), (130, 6, 5, 12)]      # n_chunks = X | 8 chunks, ragged, plane < 256 threads | 16 chunks
FLAT_N = [5, 92295 + 2]                                            # tail of 2 and of 362 work-groups before the padding to 16
SEG = {5: ([2, 5], [1e-2, 1e-3]), 92297: ([2, 45000, 92297], [1e-2, 1e-3, 1e-3])}


def optimiser_state(shape, sparse, n_flat, n_views, seed=0):
    """Two steps' worth of inputs: the grid (ping-pong pair, gradient, moments, both touched parities), the flat block, the se3
    block; gradients of the second step are kept aside because every step zeroes the ones it used."""
    X, Y, Z, C = shape
    g = torch.Generator().manual_seed(100 + seed)
    if sparse:
        p, grad, m, v, hit = K.sparse_inputs(shape, (0, X), seed)
        grad = grad * hit[..., None]                       # the engine's invariant: unmarked voxels hold a zero gradient
        hit2 = (torch.rand(X, Y, Z, generator=g) < 0.10).to(torch.uint8)
    else:
        p, grad, m, v = K.grid_inputs(shape, seed)
        hit = hit2 = None
    grad2 = torch.randn(X, Y, Z, C, generator=g) * 1e-3
    if sparse:
        grad2 = grad2 * hit2[..., None]
    r = lambda *s: torch.randn(*s, generator=g)
    seg_end, seg_lr = SEG[n_flat]
    st = dict(k0=[p, torch.full_like(p, K.CANARY)], grad=grad, m=m, v=v, tv=torch.zeros(1),
              flat_p=r(n_flat) * 0.1, flat_g=r(n_flat) * 1e-2, flat_m=r(n_flat) * 1e-3, flat_v=r(n_flat).abs() * 1e-4,
              seg_end=torch.tensor(seg_end, dtype=torch.int32), seg_lr=torch.tensor(seg_lr, dtype=torch.float32),
              se3=r(n_views * 6) * 0.01, se3_g=r(n_views * 6) * 1e-2, se3_m=r(n_views * 6) * 1e-3, se3_v=r(n_views * 6).abs() * 1e-4,
              pose_lr=torch.tensor([1e-3]))
    if sparse:
        st['touched'] = torch.stack([hit.reshape(-1), torch.zeros(X * Y * Z, dtype=torch.uint8)])
    st = {k: ([t.cuda() for t in v] if isinstance(v, list) else v.cuda()) for k, v in st.items()}
    second = dict(grad=grad2.cuda(), flat_g=(r(n_flat) * 1e-2).cuda(), se3_g=(r(n_views * 6) * 1e-2).cuda(),
                  hit=None if hit2 is None else hit2.reshape(-1).cuda())
    return st, second


def copy_state(st):
    return {k: ([t.clone() for t in v] if isinstance(v, list) else v.clone()) for k, v in st.items()}


def optimiser_steps(st, second, shape, optimize_pose, fused, rays=None):
    """Two consecutive optimiser steps on `st` (in place); -> snapshots after each step."""
    from poseprobe_amd import ops
    X, Y, Z, C = shape
    snaps = []
    for s in range(2):
        src, dst = st['k0'][s % 2], st['k0'][1 - s % 2]
        if s == 1:
            st['grad'].copy_(second['grad']); st['flat_g'].copy_(second['flat_g'])
            if rays is None:
                st['se3_g'].copy_(second['se3_g'])
            if 'touched' in st:
                st['touched'][1].copy_(second['hit'])
        grid = (src, dst, st['grad'], st['m'], st['v'], (X, Y, Z), C, 0, X, K.TV_SCALE, 0.5, K.LR, *ADAM, 3 + s, st['tv'])
        maps = (st['touched'][s % 2], st['touched'][1 - s % 2]) if 'touched' in st else None
        tail = None
        if fused:
            pose = None
            if optimize_pose or rays is not None:
                pose = (st['se3'], st['se3_g'], st['se3_m'], st['se3_v'], st['pose_lr'], *POSE_ADAM, optimize_pose)
            tail = dict(flat=(st['flat_p'], st['flat_g'], st['flat_m'], st['flat_v'], st['seg_end'], st['seg_lr'], *ADAM), pose=pose,
                        rays=None if rays is None else rays(st, s))
        elif rays is not None:
            rays(st, s, separate=True)
        if maps is None:
            ops.grid_tv_adam_step(*grid, tail=tail)
        else:
            ops.grid_tv_adam_step_sparse(*grid, *maps, tail=tail)
        if not fused:
            ops.adam_flat(st['flat_p'], st['flat_g'], st['flat_m'], st['flat_v'], st['seg_end'], st['seg_lr'], 0.5, *ADAM, 3 + s, 1)
            if optimize_pose:
                ops.adam_flat(st['se3'], st['se3_g'], st['se3_m'], st['se3_v'], torch.tensor([st['se3'].numel()], dtype=torch.int32,
                              device='cuda'), st['pose_lr'], 0.5, *POSE_ADAM, 3 + s, 1)
        torch.cuda.synchronize()
        snaps.append(copy_state(st))
    return snaps


GRID_EXACT = ('grad', 'm', 'v', 'touched', 'flat_p', 'flat_g', 'flat_m', 'flat_v')
SE3 = ('se3', 'se3_g', 'se3_m', 'se3_v')


def compare_grid(a, b, what):
    for k in GRID_EXACT:
        if k in a:
            same_bits(a[k], b[k], f'{what} {k}')
    for i in range(2):
        same_bits(a['k0'][i], b['k0'][i], f'{what} k0[{i}]')
    # tv_out: the same per-work-group sums, added by float atomics in another order
    assert_close(a['tv'].cpu(), b['tv'].cpu().double(), atol=0.0, name=f'{what} tv_out', **K.TOL['grid.tv'])


@pytest.mark.parametrize('optimize_pose', [True, False], ids=['pose', 'nopose'])
@pytest.mark.parametrize('n_flat', FLAT_N)
@pytest.mark.parametrize('sparse', [False, True], ids=['dense', 'sparse'])
@pytest.mark.parametrize('shape', GRID_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_grid_pass_with_adam_tail_equals_the_separate_launches(shape, sparse, n_flat, optimize_pose):
    """Form (a): the flat-block Adam and the se3 Adam as roles of the grid pass's launch, two consecutive steps."""
    st0, second = optimiser_state(shape, sparse, n_flat, 3)
    sep = optimiser_steps(copy_state(st0), second, shape, optimize_pose, fused=False)
    fus = optimiser_steps(copy_state(st0), second, shape, optimize_pose, fused=True)
    for s in range(2):
        compare_grid(fus[s], sep[s], f'step {s}')
        for k in SE3:
            same_bits(fus[s][k], sep[s][k], f'step {s} {k}')
    assert float(sep[1]['flat_g'].abs().max()) == 0.0 and not torch.equal(sep[1]['flat_p'], st0['flat_p'])
    if optimize_pose:
        assert float(sep[1]['se3_g'].abs().max()) == 0.0 and not torch.equal(sep[1]['se3'], st0['se3'])
    else:
        same_bits(sep[1]['se3'], st0['se3'], 'se3 without optimize_pose')


# ----------------------------------------------------------------------------------------------------------------- form (b)
def ray_inputs(V, N, seed=0):
    """N rays of V views (H = W = 8) with 0 to 11 samples each - about a fifth of the rays have none -; with V = 3 no ray looks
    through view 1.  Two sets of sample-level gradients, one per step."""
    from poseprobe_amd import ops
    H = W = 8
    g = torch.Generator().manual_seed(300 + seed)
    sc = scene((24, 24, 24))
    views = torch.tensor([0, 2] if V == 3 else list(range(V)))
    idx = (views[torch.randint(0, len(views), (N,), generator=g)] * H * W + torch.randint(0, H * W, (N,), generator=g)).int()
    rot = torch.linalg.qr(torch.randn(V, 3, 3, generator=g))[0]
    c2w = torch.cat([rot, torch.randn(V, 3, 1, generator=g) * 0.1 + torch.tensor([[0.0], [0.0], [-2.0]])], -1).contiguous()
    intr = torch.tensor([[10.0, 11.0, 4.0, 4.0]]).repeat(V, 1)
    n = torch.randint(0, 12, (N,), generator=g)
    n[torch.rand(N, generator=g) < 0.2] = 0
    n[0] = 0 if N > 1 else 5
    rs = torch.cat([torch.zeros(1, dtype=torch.long), n.cumsum(0)]).int()
    M = max(1, int(rs[-1]))
    d = dict(sc=sc, V=V, N=N, H=H, W=W, idx=idx.cuda(), c2w=c2w.cuda(), intr=intr.cuda(), rs=rs.cuda(),
             t_min=(torch.rand(N, generator=g) + 0.5).cuda(), step=torch.rand(M, generator=g).cuda(),
             jac=torch.randn(V, 12, 6, generator=g).cuda(),
             pts_grad=[torch.randn(M, 3, generator=g).cuda() for _ in range(2)],
             vgrad=[torch.randn(M, 3, generator=g).cuda() for _ in range(2)])
    z = lambda *s: torch.zeros(*s, device='cuda')
    d['rays_o'], d['rays_d'], d['viewdirs'] = z(N, 3), z(N, 3), z(N, 3)
    images, masks = z(V, H, W, 3), z(V, H, W)
    ops.raygen_select_fwd(sc, d['idx'], d['c2w'], d['intr'], H, W, True, True, images, masks, d['rays_o'], d['rays_d'], d['viewdirs'],
                          z(N, 3), z(N))
    return d


@pytest.mark.parametrize('optimize_pose', [True, False], ids=['pose', 'nopose'])
@pytest.mark.parametrize('N', [1, 7, 1024])
@pytest.mark.parametrize('V', [1, 3])
def test_ray_and_pose_backward_in_the_optimiser_launch(V, N, optimize_pose):
    """Form (b): ray backward as roles, pose backward + se3 Adam in the last work-group to arrive, against memset + ray backward +
    pose backward + grid pass + two Adam launches; two consecutive steps, so the second one starts from the c2w_grad and the arrival
    counter the first one left.  c2w_grad is a float atomic sum over rays: the four rays of a work-group add into LDS in the order
    their wavefronts arrive, the work-groups into memory likewise - so only a single ray gives the same bits in two runs of ANY of
    the two routes (7 rays did differ in one se3_grad entry on an MI355X).  Beyond one ray, c2w_grad differs by at most 64 ulps of
    its largest entry per view (the bound of test_hip_stage_kernels against its reference), which reaches se3_grad through |jac|
    and Adam's m, v and p through their first derivatives (evaluated in float64 from the separate launches' values); what the
    first step left in m, v and p is carried into the second step's bounds (m by beta1, v by beta2, p as it is)."""
    from poseprobe_amd import ops
    d = ray_inputs(V, N)
    shape = (5, 4, 3, 12)
    st0, second = optimiser_state(shape, False, 5, V)
    c2w_grad = [torch.zeros(V, 3, 4, device='cuda') for _ in range(2)]         # [0]: separate launches, [1]: fused
    arrive = torch.zeros(1, dtype=torch.int32, device='cuda')
    seen = []

    def rays(st, s, separate=False):
        a = (d['sc'], d['idx'], d['c2w'], d['intr'], d['H'], d['W'], True, d['rays_o'], d['rays_d'], d['t_min'], d['rs'],
             d['pts_grad'][s], d['step'], d['vgrad'][s])
        if not separate:
            return a + (d['jac'], c2w_grad[1], arrive)
        ops.raygen_select_bwd(*a, None, None, None, None, None, None, None, c2w_grad[0])
        ops.pose_bwd(d['jac'], c2w_grad[0], st['se3_g'].view(V, 6))
        seen.append((c2w_grad[0].clone(), st['se3_g'].clone(), st['se3_m'].clone(), st['se3_v'].clone()))

    sep = optimiser_steps(copy_state(st0), second, shape, optimize_pose, fused=False, rays=rays)
    fus = optimiser_steps(copy_state(st0), second, shape, optimize_pose, fused=True, rays=rays)
    assert float(c2w_grad[1].abs().max()) == 0.0 and int(arrive[0]) == 0, 'c2w_grad / arrival counter not left zero'
    exact = N == 1
    jabs = d['jac'].double().abs()                                                        # [V,12,6]
    dm_prev = dv_prev = dp_prev = torch.zeros(V * 6, dtype=torch.float64)
    for s in range(2):
        compare_grid(fus[s], sep[s], f'step {s}')
        cg, g, m0, v0 = (t.double().cpu() for t in seen[s])
        assert float(cg.abs().max()) > 0
        if exact:
            for k in SE3:
                same_bits(fus[s][k], sep[s][k], f'step {s} {k}')
            continue
        d_c2w = 64 * EPS * cg.abs().reshape(V, 12).max(1, keepdim=True).values.expand(V, 12)      # [V,12]
        dg = (jabs.cpu() * d_c2w[:, :, None]).sum(1).reshape(-1) + 4 * EPS * g.abs()               # [V*6]
        F, S = (fus[s][k].double().cpu() for k in SE3), (sep[s][k].double().cpu() for k in SE3)
        (fp, fg, fm, fv), (sp, sg, sm, sv) = F, S
        if not optimize_pose:
            print(f'step {s}: se3_grad max |fused - separate| {float((fg - sg).abs().max()):.3e}, bound {float(dg.max()):.3e}')
            assert bool(((fg - sg).abs() <= dg).all()), 'se3_grad'
            for k in ('se3', 'se3_m', 'se3_v'):
                same_bits(fus[s][k], sep[s][k], f'step {s} {k}')
            continue
        b1, b2, eps = POSE_ADAM
        gs = 0.5                                                                          # grad_scale of optimiser_steps
        dm = b1 * dm_prev + (1 - b1) * gs * dg + 4 * EPS * sm.abs()
        dv = b2 * dv_prev + (1 - b2) * gs * gs * (2 * g.abs() * dg + dg * dg) + 4 * EPS * sv.abs()
        step = 3 + s
        a = 1e-3 / (1 - b1 ** step)
        c = 1 / np.sqrt(1 - b2 ** step)
        den = sv.clamp_min(0).sqrt() * c + eps
        dp = dp_prev + a * (dm / den + sm.abs() * c * dv / (2 * (sv - dv).clamp_min(1e-30).sqrt() * den * den)) + 8 * EPS * (sp.abs() + a)
        dm_prev, dv_prev, dp_prev = dm, dv, dp
        for name, x, y, bound in (('se3_m', fm, sm, dm), ('se3_v', fv, sv, dv), ('se3', fp, sp, dp)):
            print(f'step {s}: {name} max |fused - separate| {float((x - y).abs().max()):.3e}, bound {float(bound.max()):.3e}')
            assert bool(((x - y).abs() <= bound).all()), name
        assert float(fg.abs().max()) == 0.0 and float(sg.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------- colour || geometry forward
SAMPLES = [1, 17, 513, 4099]      # fewer than one work-group, ragged, more than one work-group per role, sixteen per role


def sample_inputs(M, seed=0):
    """M samples of a 24^3 scene, capacity M + 37 with stale rows past the count.  A quarter of the points lie exactly on a face
    of the bounding box (some on an edge or a corner), where the trilinear stencil has out-of-range corners; the warp moves
    another part of them outside the box."""
    g = torch.Generator().manual_seed(500 + seed)
    cap = M + 37
    lo, hi = torch.tensor(XYZ_MIN), torch.tensor(XYZ_MAX)
    pts = lo + (hi - lo) * torch.rand(cap, 3, generator=g)
    face = torch.rand(cap, 3, generator=g) < 0.1
    face[::4, 0] = True
    side = torch.rand(cap, 3, generator=g) < 0.5
    pts = torch.where(face & side, lo.expand(cap, 3), torch.where(face & ~side, hi.expand(cap, 3), pts)).float()
    N = max(1, M // 7)
    wo = torch.randn(cap, 16, generator=g) * 0.05
    vd = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    d = dict(M=M, cap=cap, pts=pts, wo=wo, vd=vd, ray_id=torch.randint(0, N, (cap,), generator=g).int(),
             sdf=torch.randn(24, 24, 24, generator=g) * 0.6, ab=torch.tensor([0.35, 0.42]), k0=torch.randn(24, 24, 24, 12, generator=g),
             pe_w=torch.rand(6, generator=g), cnt=torch.tensor([M], dtype=torch.int32))
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


@pytest.mark.parametrize('M', SAMPLES)
def test_colour_lookup_beside_the_geometry_forward(M):
    """pp_geometry_color_feat_fwd against pp_geometry_fwd + pp_color_feat_fwd: no atomics, every output bit-identical, rows past
    the count untouched."""
    from poseprobe_amd import ops
    d = sample_inputs(M, seed=1)
    sc = scene((24, 24, 24))
    cap = d['cap']

    def run(fused):
        o = {k: torch.full(s, 1234.5, device='cuda') for k, s in (('alpha', (cap,)), ('gradient', (cap, 3)), ('sdf_final', (cap,)),
                                                                   ('sdf_deform', (cap,)), ('grad_deform', (cap, 9)), ('feat', (cap, 64)))}
        geo = (sc, d['sdf'], d['ab'], d['pts'], d['wo'], d['vd'], d['ray_id'], d['cnt'], cap, 37.0, o['alpha'], o['gradient'],
               o['sdf_final'], o['sdf_deform'], o['grad_deform'])
        if fused:
            ops.geometry_color_feat_fwd(*geo, d['k0'], d['pe_w'], o['feat'])
        else:
            ops.geometry_fwd(*geo)
            ops.color_feat_fwd(sc, d['k0'], d['pts'], d['vd'], d['ray_id'], o['gradient'], d['pe_w'], d['cnt'], cap, o['feat'])
        torch.cuda.synchronize()
        return o

    sep, fus = run(False), run(True)
    for k in sep:
        same_bits(fus[k], sep[k], k)
    feat = sep['feat'].cpu()
    assert bool((feat[M:] == 1234.5).all()) and bool((feat[:M, 57:] == 0).all())
    # every column is in use; a single sample on a face xyz_min has t = 0 on that axis (its t and five sines are zero): k0 and normal only
    filled = (feat[:M, :57] != 0).any(0)
    assert bool(filled.all()) if M > 1 else bool(filled[:12].all() and filled[54:57].all())


# --------------------------------------------------------------------------------------------------------------- engine level
def small_engine(**kw):
    from oracle import voxurf_oracle as O
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    G, H, W, N, V = 16, 24, 24, 96, 3
    rs = syn.range_shape()
    views = syn.make_views(V, H, W)
    idx, jit = syn.step_randomness(V * H * W, N, seed=1)
    scn = O.Scene(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, output_range=float(rs.max()), rect_size=rs.tolist())
    P = O.init_params(scn, seed=2)
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max()))
    eng = TrainEngine(cfg, V, H, W, N, device='cuda:0', **kw)
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    eng.zero_grads()
    return eng, torch.tensor(idx, dtype=torch.int32, device='cuda:0'), torch.tensor(jit, device='cuda:0')


FUSED = {'pp_grid_tv_adam_step_tail', 'pp_geometry_color_feat_fwd'}
REPLACED = {'pp_adam_flat', 'pp_pose_bwd', 'pp_raygen_select_bwd', 'pp_geometry_fwd', 'pp_color_feat_fwd', 'pp_grid_tv_adam_step_sparse'}


def test_only_the_default_path_takes_the_fused_launches(monkeypatch):
    """Calls counted through a recorder around _lib.call.  Default engine: the two fused launches replace eight separate ones (the
    memset of c2w_grad is not a library call and is not counted).
    deterministic=True and a forward with a before_k0_use hook keep the separate launches; render_and_grads on its own (callers that
    need se3_grad when it returns) keeps the separate ray / pose backward, and the next train step still finds c2w_grad clean."""
    from poseprobe_amd import _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])

    eng, idx, jit = small_engine()
    eng.train_step(idx, jit, 10)
    torch.cuda.synchronize()
    got = set(names)
    assert FUSED <= got and not (REPLACED & got), sorted(got)
    assert all(names.count(n) == 1 for n in FUSED)
    assert float(eng.c2w_grad.abs().max()) == 0.0 and int(eng.tail_arrive[0]) == 0 and float(eng.se3_grad.abs().max()) == 0.0
    assert bool(torch.isfinite(eng.se3).all()) and float(eng.se3_m.abs().max()) > 0

    names.clear()
    eng.render_and_grads(idx, jit, 11)                      # not deferred: se3_grad is complete on return, c2w_grad holds its sums
    torch.cuda.synchronize()
    assert {'pp_raygen_select_bwd', 'pp_pose_bwd'} <= set(names) and float(eng.se3_grad.abs().max()) > 0
    want = eng.se3_grad.clone()
    eng.optimizer_step(optimize_pose=False)                 # form (a) only: se3_grad untouched
    same_bits(eng.se3_grad, want, 'se3_grad after optimizer_step(optimize_pose=False)')
    names.clear()
    assert float(eng.c2w_grad.abs().max()) > 0
    eng.train_step(idx, jit, 12, optimize_pose=False)       # form (b) after a separate ray backward: c2w_grad is cleaned first
    torch.cuda.synchronize()
    assert 'pp_grid_tv_adam_step_tail' in names and 'pp_raygen_select_bwd' not in names
    assert float(eng.c2w_grad.abs().max()) == 0.0 and int(eng.tail_arrive[0]) == 0
    # the workspace still holds the step's backward: the separate launches on it give the se3_grad the fused launch left, up to
    # the order of c2w_grad's atomic sum (64 ulps of its largest entry per view, carried through |jac|)
    from poseprobe_amd import ops
    ws, cg, sg = eng.ws, torch.zeros_like(eng.c2w_grad), torch.zeros_like(eng.se3_grad)
    ops.raygen_select_bwd(eng.cfg.pp, idx, eng.c2w, eng.intr, eng.H, eng.W, eng.cfg.inverse_y, ws.rays_o, ws.rays_d, ws.t_min,
                          ws.ray_start, ws.g_pts, ws.step, ws.g_view_s, None, None, None, None, None, None, None, cg)
    ops.pose_bwd(eng.jac, cg, sg)
    torch.cuda.synchronize()
    d_c2w = 64 * EPS * cg.double().abs().reshape(eng.V, 12).max(1, keepdim=True).values.expand(eng.V, 12)
    bound = (eng.jac.double().abs() * d_c2w[:, :, None]).sum(1) + 4 * EPS * sg.double().abs()
    assert float(sg.abs().max()) > 0 and bool(((eng.se3_grad.double() - sg.double()).abs() <= bound).all())

    names.clear()
    with eng.core.pass_scope(eng.flat, eng.mlp_pack, eng.ws):
        P = eng.flat
        eng.core.forward(eng.ws, eng.k0_cl, eng.sdf, P.view('sdf_ab'), P.view('rgbnet'), P.view('warp'), 3.0, eng.pe_w,
                         before_k0_use=lambda: names.append('hook'), side_by_side=True)
    torch.cuda.synchronize()
    i = [names.index(n) for n in ('pp_geometry_fwd', 'hook', 'pp_color_feat_fwd')]
    assert i == sorted(i) and 'pp_geometry_color_feat_fwd' not in names

    names.clear()
    det, idx, jit = small_engine(deterministic=True)
    det.train_step(idx, jit, 10)
    torch.cuda.synchronize()
    got = set(names)
    assert not (FUSED & got), sorted(got)
    assert {'pp_adam_flat', 'pp_pose_bwd', 'pp_raygen_select_bwd_ordered', 'pp_k0_scatter_samples_sorted', 'pp_geometry_bwd_priors_ordered',
            'pp_geometry_fwd', 'pp_color_feat_fwd', 'pp_grid_tv_adam_step_sparse'} <= got
    assert names.count('pp_adam_flat') == 2
