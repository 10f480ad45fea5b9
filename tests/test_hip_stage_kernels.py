"""Stage kernels of the object branch, one at a time, against float64 autograd references (tests/stage_reference.py).

Accuracy rule: |hip - ref64| <= 2 |ref32 - ref64| + floor, where ref32 is the same reference evaluated in float32 on the CPU and
floor is a few float32 ulps of the largest term of the row.  So every kernel must be as accurate as a straightforward fp32
evaluation of the same maths.  Bit-exact promises (transmittance weights, T, i_end, crossing indices) are asserted as equality.

Inputs are built here (seeded).  Points are kept at least 1e-3 voxel away from integer voxel coordinates, where the float32
and float64 floors could differ; exact faces (p = xyz_min or xyz_max) are exact in both precisions and are tested as well.
Rows past `count` are filled with sentinels and must come back unchanged.
"""
import numpy as np
import pytest
import torch

from tests import stage_reference as SR
from tests.helpers import EPS, check, cu, npf  # noqa: F401  (EPS: imported from here by other test modules)

pytestmark = pytest.mark.gpu

SENT = 1234.5
XYZ_MIN = np.array([-0.6, -0.55, -0.7], np.float32)
XYZ_MAX = np.array([0.6, 0.5, 0.45], np.float32)


def rowmax(*xs):
    """Largest |value| of each row over several [M, ...] arrays -> [M, 1]."""
    return np.max(np.concatenate([np.abs(npf(x)).reshape(len(npf(x)), -1) for x in xs], 1), 1, keepdims=True)


def scene(world_size, k0_dim=12, pos_pe=5, view_pe=1, stepsize=0.5):
    from poseprobe_amd import ops
    vox = float(np.prod(XYZ_MAX - XYZ_MIN) / np.prod(world_size)) ** (1 / 3)
    return ops.make_scene(XYZ_MIN, XYZ_MAX, world_size, vox, stepsize, 0.24, 4.8, 0.0, k0_dim=k0_dim, pos_pe=pos_pe,
                          view_pe=view_pe)


def to_world(u, size):
    """Voxel coordinates [M,3] -> float32 world points."""
    size = np.asarray(size, np.float64)
    return (XYZ_MIN + u / (size - 1) * (XYZ_MAX - XYZ_MIN).astype(np.float64)).astype(np.float32)


def voxel_u(p, size):
    p = np.asarray(p, np.float64)
    return SR.grid_u(p, XYZ_MIN.astype(np.float64), XYZ_MAX.astype(np.float64), np.asarray(size, np.float64))


def off_integer(p, size, margin=1e-3):
    """True for points whose voxel coordinates are all at least `margin` from an integer."""
    u = voxel_u(p, size)
    return (np.abs(u - np.round(u)) >= margin).all(-1)


def with_sentinels(x, capacity, value=SENT):
    x = np.asarray(x)
    out = np.full((capacity,) + x.shape[1:], value, x.dtype)
    out[:len(x)] = x
    return out


def assert_untouched(name, t, count):
    rest = t.detach().cpu().numpy()[count:]
    assert (rest == SENT).all(), f'{name}: rows past count were written'


# ------------------------------------------------------------------------------------------------------------------ geometry
GEO_SIZES = [1, 255, 256, 257, 511, 512, 513, 70001]


def geo_inputs(M, world_size=(13, 7, 22), seed=0, big_deform=True):
    """Samples inside the grid, warped up to 3 voxels outside it on every face, random warp Jacobians, viewdirs of both cos
    signs plus zero viewdirs (cos exactly 0)."""
    rng = np.random.RandomState(seed)
    sz = np.array(world_size)
    N = max(1, M // 7)
    up = rng.uniform(0, sz - 1, (M, 3))
    uq = up + rng.normal(0, 0.2, (M, 3))
    if big_deform:
        far = rng.rand(M) < 0.4
        uq[far] = rng.uniform(-3, sz - 1 + 3, (far.sum(), 3))
    for _ in range(20):                    # nudge p and q off integer voxel coordinates (in float32 world coordinates)
        p = to_world(up, sz)
        q = to_world(uq, sz)
        dq = (q.astype(np.float64) - p)
        wo3 = dq.astype(np.float32)
        qq = (p + wo3).astype(np.float32)
        bad_p, bad_q = ~off_integer(p, sz), ~(off_integer(qq, sz) & off_integer(p.astype(np.float64) + wo3, sz))
        if not (bad_p.any() or bad_q.any()):
            break
        up[bad_p] += 0.0137
        uq[bad_q] += 0.0119
    assert not (bad_p.any() or bad_q.any())
    wo = np.zeros((M, 16), np.float32)
    wo[:, :3] = wo3
    wo[:, 3] = rng.normal(0, 0.05, M)
    wo[:, 4:] = rng.normal(0, 0.15, (M, 12))
    vd = rng.normal(size=(N, 3))
    vd /= np.linalg.norm(vd, axis=1, keepdims=True)
    vd[::5] = 0.0
    ray_id = rng.randint(0, N, M).astype(np.int32)
    grid = (rng.normal(0, 0.6, tuple(sz))).astype(np.float32)
    sdf_ab = np.array([0.35, 0.42], np.float32)
    return dict(p=p, wo=wo, vd=vd.astype(np.float32), ray_id=ray_id, grid=grid, sdf_ab=sdf_ab, size=tuple(int(s) for s in sz))


def geo_upstream(M, which, seed=1):
    rng = np.random.RandomState(seed)
    g = dict(g_alpha=rng.normal(size=M), g_gradient=rng.normal(size=(M, 3)), g_sdf_final=rng.normal(size=M),
             g_sdf_deform=rng.normal(size=M), g_grad_deform=rng.normal(size=(M, 9)), g_correction=rng.normal(size=M))
    g = {k: v.astype(np.float32) for k, v in g.items()}
    return g if which == 'all' else {which: g[which]}


def geo_ref(inp, sc, inv_s, up, priors=None):
    dist = float(np.float32(sc.stepsize) * np.float32(sc.voxel_size))
    return [SR.geometry(inp['p'], inp['wo'], inp['vd'], inp['ray_id'], inp['grid'], inp['sdf_ab'], inv_s, dist, XYZ_MIN,
                        XYZ_MAX, dtype=dt, priors=priors, **up) for dt in (torch.float64, torch.float32)]


def run_geometry(inp, sc, inv_s, count, capacity, up=None, priors=None, accumulate=0, prefill=None):
    """Launch pp_geometry_fwd and pp_geometry_bwd(_priors) with sentinel rows past count."""
    from poseprobe_amd import ops
    c = lambda x, v=SENT: cu(with_sentinels(x, capacity, v))
    p, wo = c(inp['p'], 0.25), c(inp['wo'], 0.01)
    ray_id = cu(with_sentinels(inp['ray_id'], capacity, 0), torch.int32)
    vd, grid, ab = cu(inp['vd']), cu(inp['grid']), cu(inp['sdf_ab'])
    cnt = cu([count], torch.int32)
    o = {k: cu(np.full(s, SENT, np.float32)) for k, s in (('alpha', capacity), ('gradient', (capacity, 3)),
                                                           ('sdf_final', capacity), ('sdf_deform', capacity),
                                                           ('grad_deform', (capacity, 9)))}
    ops.geometry_fwd(sc, grid, ab, p, wo, vd, ray_id, cnt, capacity, inv_s, o['alpha'], o['gradient'], o['sdf_final'],
                     o['sdf_deform'], o['grad_deform'])
    b = {'warp_out_grad': cu(np.full((capacity, 16), SENT, np.float32)), 'sdf_ab': torch.zeros(2, device='cuda'),
         'loss': torch.zeros(8, device='cuda')}
    for k in ('pts_grad', 'vgrad_s'):
        b[k] = c(prefill[k]) if prefill is not None else cu(np.full((capacity, 3), SENT, np.float32))
    up = up or {}
    g = {k: (c(v, 0.5) if v is not None else None) for k, v in up.items()}
    if priors is None:
        ops.geometry_bwd(sc, grid, ab, p, wo, vd, ray_id, cnt, capacity, inv_s, g.get('g_alpha'), g.get('g_gradient'),
                         g.get('g_sdf_final'), g.get('g_sdf_deform'), g.get('g_grad_deform'), g.get('g_correction'),
                         accumulate, b['warp_out_grad'], b['pts_grad'], b['vgrad_s'], b['sdf_ab'])
    else:
        w_eik, w_dyn, ls, _ = priors
        ops.geometry_bwd_priors(sc, grid, ab, p, wo, vd, ray_id, cnt, capacity, inv_s, g.get('g_alpha'), g.get('g_gradient'),
                                w_eik, w_dyn, ls, accumulate, b['warp_out_grad'], b['pts_grad'], b['vgrad_s'], b['sdf_ab'],
                                b['loss'])
    torch.cuda.synchronize()
    o.update(b)
    return o


def check_geometry(o, r64, r32, count, inv_s, inp, g_alpha=None, prefill=None):
    """Floors from the largest terms: a mapped corner value is at most A / 2, and the sigmoid derivatives of NeuS alpha carry
    inv_s |g_alpha| / den (1 + num / den) (pc + nc) into the sdf gradient, which reaches the warp and point gradients through
    grad_q sdf."""
    M = count
    sl = lambda k: o[k][:M]
    A = npf(r64['A'])
    corr = np.abs(npf(inp['wo'][:, 3]))
    sdf_terms = 0.5 * A + corr
    # alpha is a sigmoid of inv_s * sdf: its rounding floor grows with inv_s times the size of the sdf terms
    check('alpha', sl('alpha'), r64['alpha'], r32['alpha'], 1.0 + inv_s * sdf_terms)
    check('gradient', sl('gradient'), r64['gradient'], r32['gradient'], rowmax(r64['gradient'], r64['grad_deform'], r64['gq']))
    check('sdf_final', sl('sdf_final'), r64['sdf_final'], r32['sdf_final'], sdf_terms)
    check('sdf_deform', sl('sdf_deform'), r64['sdf_deform'], r32['sdf_deform'], sdf_terms + 0.5 * A)
    assert np.array_equal(npf(sl('grad_deform')), npf(r32['grad_deform'])), 'grad_deform = I + warp Jacobian, exactly'
    pc, nc = npf(r64['pc']), npf(r64['nc'])
    den, num = pc + 1e-5, pc - nc + 1e-5
    ga = np.abs(npf(g_alpha)) if g_alpha is not None else 0.0
    sig = (inv_s * ga / den * (1 + np.abs(num) / den) * (pc + nc))[:, None]
    gqm = rowmax(r64['gq'])
    scale = rowmax(r64['warp_out_grad'], r64['pts_grad']) + sig * (1 + gqm) ** 2
    check('warp_out_grad', sl('warp_out_grad'), r64['warp_out_grad'], r32['warp_out_grad'], scale, ulps=16)
    pre = {k: (npf(prefill[k]) if prefill is not None else 0.0) for k in ('pts_grad', 'vgrad_s')}
    check('pts_grad', npf(sl('pts_grad')), pre['pts_grad'] + npf(r64['pts_grad']), pre['pts_grad'] + npf(r32['pts_grad']),
          scale + np.abs(pre['pts_grad']), ulps=16)
    check('vgrad_s', npf(sl('vgrad_s')), pre['vgrad_s'] + npf(r64['vgrad_s']), pre['vgrad_s'] + npf(r32['vgrad_s']),
          rowmax(r64['vgrad_s']) + sig * rowmax(r64['gradient']) + np.abs(pre['vgrad_s']), ulps=16)
    check('sdf_ab_grad', o['sdf_ab'], r64['sdf_ab'], r32['sdf_ab'], np.abs(npf(r64['sdf_ab_rows'])).sum(0), ulps=16)
    for k in ('alpha', 'gradient', 'sdf_final', 'sdf_deform', 'grad_deform', 'warp_out_grad', 'pts_grad', 'vgrad_s'):
        assert_untouched(k, o[k], count)


@pytest.mark.parametrize('M', GEO_SIZES)
@pytest.mark.parametrize('variant', ['upstream', 'priors'])
def test_geometry_fwd_bwd_match_float64_autograd(M, variant):
    """Both backward variants at sample counts around the 256 / 512-thread work-group edges and at ~70 k samples (hundreds of
    sdf_ab_grad work-groups), with count < capacity, a non-cubic grid and warped points up to 3 voxels outside it."""
    sc = scene((13, 7, 22))
    inp = geo_inputs(M, seed=M)
    inv_s = 37.0
    if variant == 'priors':
        priors = (0.7, 0.05, 0.1, M)
        up = geo_upstream(M, 'all')
        up = {'g_alpha': up['g_alpha'], 'g_gradient': up['g_gradient']}
    else:
        priors, up = None, geo_upstream(M, 'all')
    r64, r32 = geo_ref(inp, sc, inv_s, up, priors)
    o = run_geometry(inp, sc, inv_s, M, M + 37, up=up, priors=priors)
    check_geometry(o, r64, r32, M, inv_s, inp, up.get('g_alpha'))
    if priors is not None:
        lo = o['loss'].cpu().numpy()
        check('losses', lo[2:6], r64['losses'], r32['losses'], npf(r64['losses']), ulps=64)


@pytest.mark.parametrize('which', ['g_alpha', 'g_gradient', 'g_sdf_final', 'g_sdf_deform', 'g_grad_deform', 'g_correction'])
def test_geometry_backward_of_each_upstream_input_alone(which):
    M = 513
    sc = scene((13, 7, 22))
    inp = geo_inputs(M, seed=3)
    up = geo_upstream(M, which)
    inv_s = 37.0
    r64, r32 = geo_ref(inp, sc, inv_s, up)
    full = {k: up.get(k) for k in ('g_alpha', 'g_gradient', 'g_sdf_final', 'g_sdf_deform', 'g_grad_deform', 'g_correction')}
    o = run_geometry(inp, sc, 37.0, M, M + 3, up=full)
    check_geometry(o, r64, r32, M, inv_s, inp, up.get('g_alpha'))


@pytest.mark.parametrize('variant', ['upstream', 'priors'])
def test_geometry_backward_accumulates_into_prefilled_gradients(variant):
    M = 300
    sc = scene((9, 11, 8))
    inp = geo_inputs(M, world_size=(9, 11, 8), seed=5)
    rng = np.random.RandomState(6)
    pre = {'pts_grad': rng.normal(size=(M, 3)).astype(np.float32), 'vgrad_s': rng.normal(size=(M, 3)).astype(np.float32)}
    up = geo_upstream(M, 'all')
    priors = None
    if variant == 'priors':
        priors, up = (1.0, 0.1, 0.5, M), {'g_alpha': up['g_alpha'], 'g_gradient': up['g_gradient']}
    r64, r32 = geo_ref(inp, sc, 37.0, up, priors)
    o = run_geometry(inp, sc, 37.0, M, M + 5, up=up, priors=priors, accumulate=1, prefill=pre)
    check_geometry(o, r64, r32, M, 37.0, inp, up.get('g_alpha'), prefill=pre)


def test_geometry_alpha_clip_and_cos_gate_branches():
    """inv_s large enough that the sigmoids saturate and the unclipped alpha reaches the clip bounds; cos < 0, > 0 and == 0
    (zero viewdirs) all present.  The clip passes the gradient on the closed interval, like torch.clamp."""
    M = 2000
    sc = scene((13, 7, 22))
    inp = geo_inputs(M, seed=11, big_deform=False)
    up = geo_upstream(M, 'all')
    for inv_s in (37.0, 4e4):
        r64, r32 = geo_ref(inp, sc, inv_s, up)
        cos = npf(r64['cos'])
        assert (cos < 0).any() and (cos > 0).any() and (cos == 0).sum() >= M // 10
        if inv_s > 1e3:
            a = npf(r32['a_un'])
            assert ((a <= 0) | (a >= 1)).sum() > M // 10, 'the saturated case must reach the clip bounds'
        o = run_geometry(inp, sc, inv_s, M, M, up=up)
        check_geometry(o, r64, r32, M, inv_s, inp, up.get('g_alpha'))


def test_geometry_with_zero_count_writes_nothing():
    sc = scene((13, 7, 22))
    inp = geo_inputs(64, seed=2)
    o = run_geometry(inp, sc, 37.0, 0, 64, up=geo_upstream(64, 'all'))
    for k in ('alpha', 'gradient', 'sdf_final', 'sdf_deform', 'grad_deform', 'warp_out_grad', 'pts_grad', 'vgrad_s'):
        assert_untouched(k, o[k], 0)
    assert (o['sdf_ab'].cpu().numpy() == 0).all()
    o = run_geometry(inp, sc, 37.0, 0, 64, up=geo_upstream(64, 'all'), priors=(1.0, 0.1, 1.0, 1))
    assert (o['sdf_ab'].cpu().numpy() == 0).all() and (o['loss'].cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------------------------ colour
def color_inputs(M, C, Lp, Lv, size, seed=0):
    rng = np.random.RandomState(seed)
    sz = np.array(size)
    N = max(1, M // 5)
    u = rng.uniform(0, sz - 1, (M, 3))
    k = M // 8
    u[:k] = np.where(rng.rand(k, 3) < 0.5, rng.uniform(-2, 0, (k, 3)), rng.uniform(sz - 1, sz + 1, (k, 3)))   # up to 2 voxels out
    p = to_world(u, sz)
    for _ in range(20):
        bad = ~off_integer(p, sz)
        if not bad.any():
            break
        u[bad] += 0.0131
        p = to_world(u, sz)
    assert not bad.any()
    for a in range(3):                      # exact faces: u exactly 0 or size-1 in both precisions
        p[k + 2 * a, a] = XYZ_MIN[a]
        p[k + 2 * a + 1, a] = XYZ_MAX[a]
    g = rng.normal(size=(M, 3)).astype(np.float32)
    g[1::9] = 0.0
    g[2::9] *= 1e-6 / np.linalg.norm(g[2::9], axis=1, keepdims=True)
    vd = rng.normal(size=(N, 3))
    vd = (vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32)
    pe_w = rng.uniform(0.2, 1, Lp + Lv).astype(np.float32)
    pe_w[Lp - 1] = 0.0                      # coarse-to-fine: the highest frequencies still off
    if Lv > 1:
        pe_w[Lp + Lv - 1] = 0.0
    k0 = rng.normal(size=(C,) + tuple(size)).astype(np.float32)
    fg = rng.normal(size=(M, SR.FEAT_LD)).astype(np.float32)
    return dict(p=p, g=g, vd=vd, ray_id=rng.randint(0, N, M).astype(np.int32), pe_w=pe_w, k0=k0, fg=fg)


@pytest.mark.parametrize('C,Lp,Lv', [(12, 5, 1), (8, 4, 2), (16, 3, 0)])
def test_color_features_fwd_bwd_match_float64_autograd(C, Lp, Lv):
    """The specialised (12, 5, 1) instantiation and two generic ones; points on the faces and 1-2 voxels outside (zeros
    padding), normals of norm 0 and 1e-6, zero coarse-to-fine weights, the k0 scatter as a dense tensor."""
    from poseprobe_amd import ops
    size = (11, 6, 9)
    M, cap = 700, 730
    inp = color_inputs(M, C, Lp, Lv, size, seed=C)
    sc = scene(size, k0_dim=C, pos_pe=Lp, view_pe=Lv)
    refs = [SR.color_feat(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], inp['g'], inp['pe_w'], Lp, Lv, XYZ_MIN, XYZ_MAX,
                          dtype=dt, feat_grad=inp['fg']) for dt in (torch.float64, torch.float32)]
    r64, r32 = refs
    absk0 = SR.color_feat(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], inp['g'], inp['pe_w'], Lp, Lv, XYZ_MIN, XYZ_MAX,
                          feat_grad=np.abs(inp['fg']))['k0_grad']
    c = lambda x, v=SENT: cu(with_sentinels(x, cap, v))
    k0_cl = cu(np.ascontiguousarray(inp['k0'].transpose(1, 2, 3, 0)))
    p, g, vd, pw = c(inp['p'], 0.1), c(inp['g'], 0.3), cu(inp['vd']), cu(inp['pe_w'])
    rid = cu(with_sentinels(inp['ray_id'], cap, 0), torch.int32)
    cnt = cu([M], torch.int32)
    feat = cu(np.full((cap, SR.FEAT_LD), SENT, np.float32))
    ops.color_feat_fwd(sc, k0_cl, p, vd, rid, g, pw, cnt, cap, feat)
    fg = c(inp['fg'], 0.7)
    k0g = torch.zeros_like(k0_cl)
    pg, gg, vg = (cu(np.full((cap, 3), SENT, np.float32)) for _ in range(3))
    ops.color_feat_bwd(sc, k0_cl, p, vd, rid, g, pw, cnt, cap, fg, k0g, pg, gg, vg)
    torch.cuda.synchronize()
    width = C + 3 + 6 * Lp + 3 + 6 * Lv + 3
    f = feat[:M].cpu().numpy()
    assert (f[:, width:] == 0).all(), 'columns past the used width are zero'
    check('feat', f, r64['feat'], r32['feat'], 1.0)
    scale = rowmax(r64['pts_grad'], np.abs(npf(inp['fg'])).sum(1, keepdims=True) * (np.array(size).max() / 1.0))
    check('pts_grad', pg[:M], r64['pts_grad'], r32['pts_grad'], scale, ulps=16)
    gn = np.linalg.norm(inp['g'].astype(np.float64), axis=1, keepdims=True)
    check('gradient_grad', gg[:M], r64['gradient_grad'], r32['gradient_grad'],
          rowmax(r64['gradient_grad'], np.abs(inp['fg'][:, width - 3:width]) / (gn + 1e-5)), ulps=16)
    check('vgrad_s', vg[:M], r64['vgrad_s'], r32['vgrad_s'], rowmax(r64['vgrad_s'], inp['fg']), ulps=16)
    to_cl = lambda x: npf(x).transpose(1, 2, 3, 0)
    check('k0_grad', k0g, to_cl(r64['k0_grad']), to_cl(r32['k0_grad']), to_cl(absk0), ulps=16)
    for k, t in (('feat', feat), ('pts_grad', pg), ('gradient_grad', gg), ('vgrad_s', vg)):
        assert_untouched(k, t, M)
    # count == 0: nothing written, nothing scattered
    feat0 = cu(np.full((cap, SR.FEAT_LD), SENT, np.float32))
    z = cu([0], torch.int32)
    ops.color_feat_fwd(sc, k0_cl, p, vd, rid, g, pw, z, cap, feat0)
    k0g.zero_()
    ops.color_feat_bwd(sc, k0_cl, p, vd, rid, g, pw, z, cap, fg, k0g, pg, gg, vg)
    torch.cuda.synchronize()
    assert_untouched('feat (count 0)', feat0, 0)
    assert (k0g.cpu().numpy() == 0).all()


# ------------------------------------------------------------------------------------------------------------------ compositing
LENS = [0, 1, 63, 64, 65, 127, 128, 129, 1000, 129, 1000, 2, 2]


def march_inputs(bg, seed=0):
    """Segments of every length around the 64-lane chunk edges; the early stop forced onto lane 63 of chunk 1 (ray 9, sample
    127) and lane 0 of chunk 2 (ray 10, sample 128); rgb_pre exactly 0 (bg 0, black ray) or exactly 1 (bg 1, dyadic weights)."""
    rng = np.random.RandomState(seed)
    lens = np.array(LENS)
    rs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    M = int(rs[-1])
    alpha = rng.uniform(0, 0.012, M).astype(np.float32)
    alpha[rs[9] + 127] = 0.9999
    alpha[rs[10] + 128] = 0.9999
    rgb = rng.uniform(0, 1, (M, 3)).astype(np.float32)
    rgb[rs[5]:rs[6]] = 0.0                  # bg 0: rgb_pre exactly 0
    alpha[rs[11]:rs[12]] = 0.5              # weights 0.5, 0.25: with bg 1 and white samples rgb_pre is exactly 1
    rgb[rs[11]:rs[12]] = 1.0
    alpha[rs[12]:rs[13]] = 0.5
    rgb[rs[12]:rs[13]] = 0.0
    N = len(lens)
    return dict(alpha=alpha, rgb=rgb, rs=rs, M=M, N=N, step_w=rng.uniform(0.1, 2, M).astype(np.float32),
                nrm=rng.normal(size=(M, 3)).astype(np.float32), g_rgbm=rng.normal(size=(N, 3)).astype(np.float32),
                g_cw=rng.normal(size=N).astype(np.float32), g_last=rng.normal(size=N).astype(np.float32),
                g_depth=rng.normal(size=N).astype(np.float32), g_w=rng.normal(size=M).astype(np.float32))


MARCH_OPTIONAL = ['step_w', 'nrm_in', 'rgb_pre', 'g_rgbm', 'g_cw', 'g_last', 'g_depth', 'g_w_in', 'g_rgb']


@pytest.mark.parametrize('bg', [0.0, 1.0])
@pytest.mark.parametrize('absent', [None] + MARCH_OPTIONAL)
def test_fused_march_fwd_bwd_match_float64_autograd(bg, absent):
    from poseprobe_amd import ops
    d = march_inputs(bg)
    M, N, rs = d['M'], d['N'], d['rs']
    has = lambda k: k != absent
    kw = dict(step_w=d['step_w'] if has('step_w') else None, nrm=d['nrm'], clamp=has('rgb_pre'),
              g_rgbm=d['g_rgbm'] if has('g_rgbm') else None, g_cw=d['g_cw'] if has('g_cw') else None,
              g_last=d['g_last'] if has('g_last') else None, g_depth=d['g_depth'] if has('g_depth') and has('step_w') else None,
              g_w=d['g_w'] if has('g_w_in') else None)
    r64, r32 = (SR.march(d['alpha'], d['rgb'], rs, bg, dtype=dt, **kw) for dt in (torch.float64, torch.float32))
    ie = r64['i_end'].numpy()
    assert ie[9] == rs[9] + 128 and ie[10] == rs[10] + 129, 'the forced stops'
    pre64 = npf(r64['rgb_pre'])
    assert (pre64 == 0).any() if bg == 0 else (pre64 == 1).any()
    a, rgb, rsd = cu(d['alpha']), cu(d['rgb']), cu(rs, torch.int32)
    w, T = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    last, cw = torch.empty(N, device='cuda'), torch.empty(N, device='cuda')
    i_end = torch.empty(N, device='cuda', dtype=torch.int32)
    opt = lambda k, shape: torch.full(shape, SENT, device='cuda') if has(k) else None
    rgbm, pre, depth, nrmm = torch.empty(N, 3, device='cuda'), opt('rgb_pre', (N, 3)), torch.empty(N, device='cuda'), \
        torch.empty(N, 3, device='cuda')
    sw = cu(d['step_w']) if has('step_w') else None
    nin = cu(d['nrm']) if has('nrm_in') else None
    ops.march_fwd(a, rgb, sw, nin, rsd, N, bg, w, T, last, i_end, rgbm, pre, cw, depth, nrmm)
    torch.cuda.synchronize()
    assert np.array_equal(w.cpu().numpy(), r64['weights32'].numpy())
    assert np.array_equal(T.cpu().numpy(), r64['T32'].numpy())
    assert np.array_equal(last.cpu().numpy(), r64['last32'].numpy())
    ne = rs[1:] > rs[:-1]
    assert np.array_equal(i_end.cpu().numpy()[ne], ie[ne])
    absw = npf(r64['weights'])
    segabs = lambda x: np.add.reduceat(np.concatenate([x, np.zeros((1,) + x.shape[1:])]), rs[:-1])
    wsum = np.where(ne, segabs(absw), 0.0)
    check('cum_weights', cw, r64['cum_weights'], r32['cum_weights'], wsum)
    check('rgb_marched', rgbm, npf(r64['rgb_pre']).clip(0, 1), npf(r32['rgb_pre']).clip(0, 1), wsum[:, None] + bg)
    if has('rgb_pre'):
        check('rgb_pre', pre, r64['rgb_pre'], r32['rgb_pre'], wsum[:, None] + bg)
    if has('step_w'):
        check('depth_acc', depth, r64['depth_acc'], r32['depth_acc'], np.where(ne, segabs(absw * d['step_w']), 0))
    if has('nrm_in'):
        check('normal_marched', nrmm, r64['normal_marched'], r32['normal_marched'],
              np.where(ne[:, None], segabs(absw[:, None] * np.abs(d['nrm'])), 0))
    # backward
    g = lambda k, name: cu(d[k]) if has(name) else None
    ga = torch.full((M,), SENT, device='cuda')
    grgb = torch.full((M, 3), SENT, device='cuda') if has('g_rgb') else None
    ops.march_bwd(a, rgb, sw, w, T, last, rsd, i_end, N, bg, pre, g('g_rgbm', 'g_rgbm'), g('g_cw', 'g_cw'),
                  g('g_last', 'g_last'), g('g_depth', 'g_depth'), g('g_w', 'g_w_in'), ga, grgb)
    torch.cuda.synchronize()
    # the scale of g_alpha_i: |total weight gradient| T_i plus the magnitude of everything behind it over (1 - alpha_i)
    ray = np.repeat(np.arange(N), np.diff(rs))
    gmag = np.abs(npf(kw['g_rgbm'] if kw['g_rgbm'] is not None else np.zeros((N, 3))))
    gw_abs = (np.abs(npf(kw['g_w'])) if kw['g_w'] is not None else 0) + (gmag[ray] * d['rgb']).sum(1) \
        + (np.abs(npf(kw['g_cw']))[ray] if kw['g_cw'] is not None else 0) + bg * gmag.sum(1)[ray] \
        + (np.abs(kw['g_depth'])[ray] * d['step_w'] if kw['g_depth'] is not None else 0)
    T64 = npf(r64['T32'])
    behind = np.zeros(M)
    gl = np.abs(npf(kw['g_last'])) if kw['g_last'] is not None else np.zeros(N)
    for k in range(N):
        b, e = rs[k], rs[k + 1]
        tail = np.cumsum((gw_abs * absw)[b:e][::-1])[::-1]
        behind[b:e] = np.concatenate([tail[1:], [0]]) + gl[k] * npf(r64['alphainv_last'])[k]
    scale = gw_abs * T64 + behind / (1 - d['alpha'].astype(np.float64))
    check('g_alpha', ga, r64['g_alpha'], r32['g_alpha'], scale, ulps=32)
    if has('g_rgb'):
        check('g_rgb', grgb, r64['g_rgb'], r32['g_rgb'], absw[:, None] * gmag[ray])


def test_dvgo_march_matches_float64_cumprod():
    """No early stop, 1 - alpha clamped to 1e-10 (alpha == 1 samples) and alpha == 0 samples; T and the weights are products,
    so they are checked relative to their own size."""
    from poseprobe_amd import ops
    d = march_inputs(0.0, seed=3)
    M, N, rs = d['M'], d['N'], d['rs']
    alpha = d['alpha'].copy()
    alpha[rs[8] + 10] = 1.0
    alpha[rs[10] + 700] = 1.0
    alpha[rs[6]:rs[6] + 40] = 0.0
    r64, r32 = (SR.march_dvgo(alpha, d['rgb'], d['step_w'], rs, dtype=dt) for dt in (torch.float64, torch.float32))
    w, T = torch.empty(M, device='cuda'), torch.empty(M, device='cuda')
    last, cw, depth = (torch.empty(N, device='cuda') for _ in range(3))
    rgb_acc = torch.empty(N, 3, device='cuda')
    i_end = torch.empty(N, device='cuda', dtype=torch.int32)
    ops.march_dvgo_fwd(cu(alpha), cu(d['rgb']), cu(d['step_w']), cu(rs, torch.int32), N, w, T, last, i_end, rgb_acc, cw, depth)
    torch.cuda.synchronize()
    ne = rs[1:] > rs[:-1]
    assert np.array_equal(i_end.cpu().numpy()[ne], rs[1:][ne])
    n_in = np.repeat(np.diff(rs), np.diff(rs)).astype(np.float64)      # products of up to n factors: n ulps
    check('T', T, r64['T'], r32['T'], np.abs(npf(r64['T'])) * n_in)
    check('weights', w, r64['weights'], r32['weights'], np.abs(npf(r64['weights'])) * n_in)
    check('alphainv_last', last, r64['alphainv_last'], r32['alphainv_last'], np.abs(npf(r64['alphainv_last'])) * np.diff(rs))
    assert (npf(r64['T'])[rs[8] + 11:rs[9]] < 1e-9).all() and (npf(T.cpu())[rs[8] + 11:rs[9]] > 0).all()
    wabs = np.abs(npf(r64['weights']))
    segabs = lambda x: np.where(ne.reshape((-1,) + (1,) * (x.ndim - 1)),
                                np.add.reduceat(np.concatenate([x, np.zeros((1,) + x.shape[1:])]), rs[:-1]), 0)
    check('cum_weights', cw, r64['cum_weights'], r32['cum_weights'], segabs(wabs))
    check('rgb_acc', rgb_acc, r64['rgb_acc'], r32['rgb_acc'], segabs(wabs[:, None] * d['rgb']))
    check('depth_acc', depth, r64['depth_acc'], r32['depth_acc'], segabs(wabs * d['step_w']))


# ------------------------------------------------------------------------------------------------------------------ rays
def ray_inputs(seed=0):
    from oracle import voxurf_oracle as O
    from poseprobe_amd import synthetic as syn
    rng = np.random.RandomState(seed)
    V, H, W = 3, 16, 16
    views = syn.make_views(V, H, W)
    c2w = O.pose_invert(torch.tensor(views['w2c'])).numpy().astype(np.float32)
    lens = np.array([0, 1, 5, 130, 0, 64, 65, 3, 1, 200, 7, 2])
    N = len(lens)
    idx = rng.randint(0, V * H * W, N).astype(np.int32)
    idx[:4] = [0, H * W + 5, 2 * H * W + 17, H * W - 1]
    rs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    M = int(rs[-1])
    step = np.concatenate([np.sort(rng.uniform(0, 1.5, n)) for n in lens]).astype(np.float32)
    return dict(V=V, H=H, W=W, Ks=views['Ks'].astype(np.float32), c2w=c2w, idx=idx, rs=rs, M=M, N=N, step=step,
                pts_grad=rng.normal(size=(M, 3)).astype(np.float32), vgrad_s=rng.normal(size=(M, 3)).astype(np.float32),
                g_depth=rng.normal(size=N).astype(np.float32))


@pytest.mark.parametrize('with_v,with_depth', [(True, True), (False, False), (True, False), (False, True)])
def test_raygen_select_bwd_c2w_gradient_matches_float64_autograd(with_v, with_depth):
    from poseprobe_amd import ops
    d = ray_inputs()
    sc = scene((16, 16, 16))
    vg, gdp = (d['vgrad_s'] if with_v else None), (d['g_depth'] if with_depth else None)
    refs = [SR.raygen_select_bwd(d['c2w'], d['Ks'], d['H'], d['W'], d['idx'], d['rs'], d['pts_grad'], d['step'], XYZ_MIN,
                                 XYZ_MAX, 0.24, 4.8, vgrad_s=vg, g_depth=gdp, dtype=dt) for dt in (torch.float64, torch.float32)]
    r64, r32 = refs
    ro, rd = r32['rays_o'].float(), r32['rays_d'].float()
    tmin = SR.slab_t_min(ro, rd, torch.tensor(XYZ_MIN), torch.tensor(XYZ_MAX), 0.24, 4.8)
    Ks = d['Ks']
    intr = cu(np.stack([Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2]], -1))
    c2w_grad = torch.full((d['V'], 3, 4), SENT, device='cuda')
    N = d['N']
    go, gd, gv = (torch.empty(N, 3, device='cuda') for _ in range(3))
    ops.raygen_select_bwd(sc, cu(d['idx'], torch.int32), cu(d['c2w']), intr, d['H'], d['W'], True, cu(ro), cu(rd), cu(tmin),
                          cu(d['rs'], torch.int32), cu(d['pts_grad']), cu(d['step']), cu(vg) if with_v else None, None, None,
                          None, cu(gdp) if with_depth else None, go, gd, gv, c2w_grad)
    torch.cuda.synchronize()
    check('c2w_grad', c2w_grad, r64['c2w_grad'], r32['c2w_grad'], rowmax(r64['c2w_grad']).reshape(-1, 1, 1), ulps=64)
    check('g_o', go, r64['g_o'], r32['g_o'], rowmax(r64['g_o'], r64['g_d']), ulps=32)
    check('g_d', gd, r64['g_d'], r32['g_d'], rowmax(r64['g_o'], r64['g_d']), ulps=32)
    check('g_v', gv, r64['g_v'], r32['g_v'], rowmax(r64['g_v']), ulps=32)


def test_raygen_select_bwd_without_cameras_adds_the_ray_upstreams():
    """The drop-in call form: no ray_idx / c2w (only the per-ray gradients), upstream ray gradients added."""
    from poseprobe_amd import ops
    d = ray_inputs(seed=4)
    sc = scene((16, 16, 16))
    r64, r32 = (SR.raygen_select_bwd(d['c2w'], d['Ks'], d['H'], d['W'], d['idx'], d['rs'], d['pts_grad'], d['step'], XYZ_MIN,
                                     XYZ_MAX, 0.24, 4.8, vgrad_s=d['vgrad_s'], g_depth=d['g_depth'], dtype=dt)
                for dt in (torch.float64, torch.float32))
    ro, rd = r32['rays_o'].float(), r32['rays_d'].float()
    tmin = SR.slab_t_min(ro, rd, torch.tensor(XYZ_MIN), torch.tensor(XYZ_MAX), 0.24, 4.8)
    N = d['N']
    rng = np.random.RandomState(9)
    up = [rng.normal(size=(N, 3)).astype(np.float32) for _ in range(3)]
    go, gd, gv = (torch.empty(N, 3, device='cuda') for _ in range(3))
    ops.raygen_select_bwd(sc, None, None, None, d['H'], d['W'], True, cu(ro), cu(rd), cu(tmin), cu(d['rs'], torch.int32),
                          cu(d['pts_grad']), cu(d['step']), cu(d['vgrad_s']), cu(up[0]), cu(up[1]), cu(up[2]), cu(d['g_depth']),
                          go, gd, gv, None)
    torch.cuda.synchronize()
    for name, t, k, u in (('g_o', go, 'g_o', up[0]), ('g_d', gd, 'g_d', up[1]), ('g_v', gv, 'g_v', up[2])):
        check(name, t, npf(r64[k]) + u, npf(r32[k]) + u, rowmax(r64[k]) + np.abs(u), ulps=32)


# ------------------------------------------------------------------------------------------------------------------ grid sample
@pytest.mark.parametrize('border', [0, 1])
@pytest.mark.parametrize('C', [1, 12])
def test_grid_sample_fwd_bwd_match_float64_grid_sample(border, C):
    from poseprobe_amd import ops
    size = (10, 7, 13)
    sz = np.array(size)
    rng = np.random.RandomState(C + border)
    M = 900
    u = rng.uniform(-2.5, sz + 1.5, (M, 3))
    u[:M // 3] = rng.uniform(0, sz - 1, (M // 3, 3))
    p = to_world(u, sz)
    for _ in range(20):
        bad = ~off_integer(p, sz)
        if not bad.any():
            break
        u[bad] += 0.0123
        p = to_world(u, sz)
    for a in range(3):
        p[2 * a, a], p[2 * a + 1, a] = XYZ_MIN[a], XYZ_MAX[a]
    grid = rng.normal(size=(C,) + size).astype(np.float32)
    og = rng.normal(size=(M, C)).astype(np.float32)
    r64, r32 = (SR.grid_sample(grid, p, XYZ_MIN, XYZ_MAX, border, dtype=dt, out_grad=og) for dt in (torch.float64, torch.float32))
    gabs = SR.grid_sample(grid, p, XYZ_MIN, XYZ_MAX, border, out_grad=np.abs(og))['grid_grad']
    sc = scene(size, k0_dim=C)
    g_cl = cu(np.ascontiguousarray(grid.transpose(1, 2, 3, 0)))
    out = torch.empty(M, C, device='cuda')
    ops.grid_sample_fwd(sc, g_cl, C, cu(p), border, out)
    gg, pg = torch.zeros_like(g_cl), torch.empty(M, 3, device='cuda')
    ops.grid_sample_bwd(sc, g_cl, C, cu(p), border, cu(og), gg, pg)
    torch.cuda.synchronize()
    check('out', out, r64['out'], r32['out'], np.abs(grid).max())
    to_cl = lambda x: npf(x).transpose(1, 2, 3, 0)
    check('grid_grad', gg, to_cl(r64['grid_grad']), to_cl(r32['grid_grad']), to_cl(gabs), ulps=16)
    scl = (sz - 1) / (XYZ_MAX - XYZ_MIN).astype(np.float64)
    check('pts_grad', pg, r64['pts_grad'], r32['pts_grad'],
          np.abs(og).sum(1, keepdims=True) * np.abs(grid).max() * scl.max(), ulps=16)


# ------------------------------------------------------------------------------------------------------------------ first crossing
def crossing_rows(S, rng):
    rows = [np.abs(rng.normal(size=S)) + 0.1]                      # no sign change
    r = np.abs(rng.normal(size=S)) + 0.1; r[1:] *= -1; rows.append(r)          # crossing at the first pair
    r = np.abs(rng.normal(size=S)) + 0.1; r[-1] *= -1; rows.append(r)          # crossing at the last pair
    r = np.abs(rng.normal(size=S)) + 0.1; r[S // 2] = 0.0; rows.append(r)      # exact zero inside
    rows.append(np.zeros(S))                                       # all zero
    r = -np.abs(rng.normal(size=S)) - 0.1; r[0] = 0.0; rows.append(r)         # zero first
    for _ in range(6):
        rows.append(np.cumsum(rng.normal(size=S) * 0.3) + rng.uniform(-1, 2))
    return np.array(rows, np.float32)


@pytest.mark.parametrize('S', [2, 65, 1024])
@pytest.mark.parametrize('compact', [False, True])
def test_sdf_first_crossing_matches_the_reference_query(S, compact):
    from poseprobe_amd import ops
    rng = np.random.RandomState(S)
    rows = crossing_rows(S, rng)
    N = len(rows)
    dist = 0.0173
    ro = rng.normal(size=(N, 3)).astype(np.float32)
    rd = rng.normal(size=(N, 3)).astype(np.float32)
    tmin = rng.uniform(0.2, 1.0, N).astype(np.float32)
    dense = rows.copy()
    pts, mask = torch.empty(N, 3, device='cuda'), torch.empty(N, device='cuda', dtype=torch.uint8)
    zval, sd = torch.empty(N, device='cuda'), torch.empty(N, S, device='cuda')
    if compact:
        keep = rng.rand(N, S) < 0.6
        keep[1] = False                                            # an empty ray
        dense = np.where(keep, rows, 1.0).astype(np.float32)
        rs = np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int32)
        step_k = np.nonzero(keep)[1].astype(np.int32)
        vals = rows[keep]
        ops.sdf_first_crossing(cu(vals if len(vals) else np.zeros(1)), cu(rs, torch.int32),
                               cu(step_k if len(step_k) else np.zeros(1, np.int32), torch.int32), N, S, dist, cu(tmin), cu(ro),
                               cu(rd), sd, pts, mask, zval)
    else:
        ops.sdf_first_crossing(cu(rows), None, None, N, S, dist, cu(tmin), cu(ro), cu(rd), sd, pts, mask, zval)
    torch.cuda.synchronize()
    assert np.array_equal(sd.cpu().numpy(), dense)
    (p64, h64), (p32, h32) = (SR.first_crossing(dense, tmin, ro, rd, dist, dtype=dt) for dt in (torch.float64, torch.float32))
    assert np.array_equal(mask.cpu().numpy().astype(bool), h64.numpy().astype(bool))
    check('pts', pts, p64, p32, np.abs(ro) + np.abs(rd) * (np.abs(tmin)[:, None] + S * dist / np.linalg.norm(rd, axis=1,
                                                                                                               keepdims=True)))
