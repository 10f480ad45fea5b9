"""The kernels behind the DirectVoxGO twin, one at a time, against float64 autograd references (tests/generic_reference.py):
the generic feature builder and its k0 backward (csrc/pp_color.hip), the generic MLP layer by layer (csrc/pp_mlp_layered.hip)
and the diffuse-logit path (logit_add / logit_add_grad) on the layered, fp32-fused and split-precision fused routes.

Where the bounds come from:
  * feature builder: the rule of tests/test_hip_stage_kernels.py, |hip - ref64| <= 2 |ref32 - ref64| + 8 ulp * scale, scale = the row's
    largest |k0 corner value| for the lookup columns, 1 for encodings and normals; the k0 scatter with 16 ulp of the sum of the
    |contributions| of a voxel, as that file's k0_grad check of the specialised builder;
  * MLP: the tolerances tests/test_hip_mlp.py applies to the rgbnet chain (values rtol 1e-4 / atol 1e-5; gradients rtol 1e-3, atol 2e-5,
    1e-3 of the tensor's largest entry), against float64.  The float32 CPU evaluation of the same reference uses at most 1.5 % of
    these bounds at every shape here (the deepest, n_gemm = 8, included: worst entry 0.015 of the value bound at 65 rows, 0.010 at
    1000), so they hold unchanged;
  * the split-precision rule of tests/test_hip_mlp.py::test_split_precision_kernels_are_as_accurate_as_the_fp32_instructions.

MLP inputs are picked by the float64 reference alone (generic_reference.pick_rows): no hidden pre-activation lies within fp32
rounding of zero, so no row is excused.  Points follow the stage tests: off-integer voxel coordinates, plus exact faces.
"""
import functools

import numpy as np
import pytest
import torch

from tests import generic_reference as GR
from tests.helpers import assert_close
from tests.test_hip_stage_kernels import (EPS, SENT, XYZ_MAX, XYZ_MIN, assert_untouched, check, cu, npf, off_integer, scene,
                                          to_world, with_sentinels)

pytestmark = pytest.mark.gpu

SIZE = (7, 5, 9)
GUARD = 4096
PREFILL = 0.125

# (C, k0_skip, Lp, Lv, ld, gradient, pe_w)
FEAT_CASES = [(12, 0, 5, 4, 96, False, False), (12, 3, 5, 4, 96, False, False), (4, 0, 5, 4, 64, False, False),
              (4, 3, 5, 4, 64, False, False), (16, 3, 2, 1, 64, False, False), (4, 3, 0, 0, 32, False, False),
              (16, 0, 5, 4, 96, True, True)]


# ------------------------------------------------------------------------------------------------------------------ features
def feat_inputs(M, case, seed=0):
    """A fifth of the points up to 2 voxels outside the box on some axes (zeros padding), a third packed into two voxel cells
    (colliding atomics in the scatter), exact faces, about 30 % of the rows switched off."""
    C, skip, Lp, Lv, ld, with_g, with_w = case
    rng = np.random.RandomState(seed)
    sz = np.array(SIZE)
    N = max(1, M // 5)
    u = rng.uniform(0, sz - 1, (M, 3))
    k, j = M // 5, M // 3
    where = rng.randint(0, 3, (k, 3))
    where[:, 0] = np.where((where == 0).all(1), 1, where[:, 0])                  # at least one axis outside
    u[:k] = np.select([where == 0, where == 1], [u[:k], rng.uniform(-2, 0, (k, 3))], rng.uniform(sz - 1, sz + 1, (k, 3)))
    u[k:k + j] = np.array([[2, 1, 3], [4, 3, 6]])[rng.randint(0, 2, j)] + rng.uniform(0.05, 0.95, (j, 3))
    p = to_world(u, sz)
    for _ in range(20):
        bad = ~off_integer(p, sz)
        if not bad.any():
            break
        u[bad] += 0.0131
        p = to_world(u, sz)
    assert not bad.any()
    if M >= k + j + 6:
        for a in range(3):                  # exact faces: u exactly 0 or size-1 in both precisions
            p[k + j + 2 * a, a] = XYZ_MIN[a]
            p[k + j + 2 * a + 1, a] = XYZ_MAX[a]
    g = rng.normal(size=(M, 3)).astype(np.float32)
    g[1::9] = 0.0
    g[2::9] *= 1e-6 / np.linalg.norm(g[2::9], axis=1, keepdims=True)
    vd = rng.normal(size=(N, 3))
    vd = (vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32)
    pe_w = rng.uniform(0.2, 1, Lp + Lv).astype(np.float32)
    if Lp + Lv:
        pe_w[-1] = 0.0
    sel = (rng.rand(M) < 0.7).astype(np.uint8)
    if M == 1:
        sel[:] = 1
    return dict(p=p, g=g if with_g else None, vd=vd, ray_id=rng.randint(0, N, M).astype(np.int32),
                pe_w=pe_w if with_w else None, sel=sel, k0=rng.normal(size=(C,) + SIZE).astype(np.float32),
                fg=rng.normal(size=(M, ld)).astype(np.float32), rg=rng.normal(size=(M, C)).astype(np.float32))


def feat_refs(inp, case, sel, **grads):
    C, skip, Lp, Lv, ld, _, _ = case
    return [GR.feat_generic(inp['k0'], inp['p'], inp['vd'], inp['ray_id'], inp['g'], inp['pe_w'], sel, skip, ld, Lp, Lv, XYZ_MIN,
                            XYZ_MAX, dtype=dt, **grads) for dt in (torch.float64, torch.float32)]


def feat_device(inp, case, rows):
    """Device copies with `rows` rows: the rows past the inputs hold values that would show in the outputs if they were read."""
    C = case[0]
    c = lambda x, v: None if x is None else cu(with_sentinels(x, rows, v))
    return dict(sc=scene(SIZE, k0_dim=C, pos_pe=case[2], view_pe=case[3]),
                k0_cl=cu(np.ascontiguousarray(inp['k0'].transpose(1, 2, 3, 0))), p=c(inp['p'], 0.1), g=c(inp['g'], 0.3),
                vd=cu(inp['vd']), pw=None if inp['pe_w'] is None else cu(inp['pe_w']),
                rid=cu(with_sentinels(inp['ray_id'], rows, 0), torch.int32), fg=c(inp['fg'], 0.7), rg=c(inp['rg'], 0.9))


def run_feat_fwd(inp, case, count, cap, rows, sel, want_raw=True):
    from poseprobe_amd import ops
    C, skip, Lp, Lv, ld, _, _ = case
    d = feat_device(inp, case, rows)
    sel_d = None if sel is None else cu(with_sentinels(sel, rows, 1), torch.uint8)
    feat = cu(np.full((rows, ld), SENT, np.float32))
    raw = cu(np.full((rows, C), SENT, np.float32)) if want_raw else None
    ops.feat_generic_fwd(d['sc'], d['k0_cl'], d['p'], d['vd'], d['rid'], d['g'], d['pw'], sel_d, skip, ld, cu([count], torch.int32),
                         cap, feat, raw)
    torch.cuda.synchronize()
    return feat, raw


def check_feat_fwd(feat, raw, inp, case, sel, M):
    C, skip, Lp, Lv, ld, _, _ = case
    r64, r32 = feat_refs(inp, case, sel)
    width = r64['width']
    assert width == C - skip + 3 + 6 * Lp + 3 + 6 * Lv + (3 if inp['g'] is not None else 0)
    cm = GR.corner_absmax(inp['k0'], inp['p'], XYZ_MIN, XYZ_MAX)
    scale = np.ones((M, ld))
    scale[:, :C - skip] = cm
    f = feat[:M].cpu().numpy()
    check('feat', f, r64['feat'], r32['feat'], scale)
    assert (f[:, width:] == 0).all(), 'columns past the used width are zero'
    off = np.zeros(M, bool) if sel is None else sel == 0
    assert (f[off] == 0).all(), 'rows with sel == 0 are zero'
    assert_untouched('feat', feat, M)
    if raw is not None:
        k = raw[:M].cpu().numpy()
        check('k0_raw', k, r64['k0_raw'], r32['k0_raw'], cm)
        assert (k[off] == 0).all(), 'k0_raw rows with sel == 0 are zero'
        on = ~off
        assert np.array_equal(k[on][:, skip:], f[on][:, :C - skip]), 'the feature columns are the lookup without its first channels'
        assert_untouched('k0_raw', raw, M)


@pytest.mark.parametrize('M', [1, 255, 256, 257])
@pytest.mark.parametrize('case', FEAT_CASES, ids=lambda c: 'C{}s{}p{}v{}ld{}{}'.format(*c[:5], 'gw' if c[5] else ''))
def test_generic_features_fwd_and_k0_bwd_match_float64_autograd(case, M):
    """pp_feat_generic_fwd and pp_feat_generic_bwd_k0 on either side of a 256-thread block, capacity = M + 3; k0_raw is left out
    once per case (M = 255)."""
    from poseprobe_amd import ops
    C, skip, Lp, Lv, ld, _, _ = case
    inp = feat_inputs(M, case, seed=M + C)
    sel = inp['sel']
    cap = M + 3
    feat, raw = run_feat_fwd(inp, case, M, cap, cap, sel, want_raw=(M != 255))
    check_feat_fwd(feat, raw, inp, case, sel, M)
    # backward: k0_grad accumulates into a pre-filled tensor; with and without the gradient of k0_raw
    d = feat_device(inp, case, cap)
    sel_d = cu(with_sentinels(sel, cap, 1), torch.uint8)
    to_cl = lambda x: npf(x).transpose(1, 2, 3, 0)
    for rg in (None, inp['rg']):
        r64, r32 = feat_refs(inp, case, sel, feat_grad=inp['fg'], k0_raw_grad=rg)
        contrib = feat_refs(inp, case, sel, feat_grad=np.abs(inp['fg']), k0_raw_grad=None if rg is None else np.abs(rg))[0]
        k0g = torch.full_like(d['k0_cl'], PREFILL)
        ops.feat_generic_bwd_k0(d['sc'], d['p'], sel_d, skip, ld, cu([M], torch.int32), cap, d['fg'], None if rg is None else d['rg'],
                                k0g)
        torch.cuda.synchronize()
        check('k0_grad', k0g, PREFILL + to_cl(r64['k0_grad']), PREFILL + to_cl(r32['k0_grad']),
              PREFILL + to_cl(contrib['k0_grad']), ulps=16)
        if rg is None and skip:
            assert (k0g[..., :skip] == PREFILL).all(), 'the skipped channels get a gradient only through k0_raw'


def test_generic_features_without_a_selection_mask():
    case, M = FEAT_CASES[1], 257
    inp = feat_inputs(M, case, seed=3)
    feat, raw = run_feat_fwd(inp, case, M, M + 3, M + 3, None)
    check_feat_fwd(feat, raw, inp, case, None, M)


def test_generic_features_clamp_the_count_to_the_capacity():
    from poseprobe_amd import ops
    case, cap = FEAT_CASES[3], 300
    C, skip, Lp, Lv, ld, _, _ = case
    inp = feat_inputs(cap, case, seed=9)
    feat, raw = run_feat_fwd(inp, case, cap + 50, cap, cap + 8, inp['sel'])
    check_feat_fwd(feat, raw, inp, case, inp['sel'], cap)
    d = feat_device(inp, case, cap + 8)
    r64, r32 = feat_refs(inp, case, inp['sel'], feat_grad=inp['fg'], k0_raw_grad=inp['rg'])
    contrib = feat_refs(inp, case, inp['sel'], feat_grad=np.abs(inp['fg']), k0_raw_grad=np.abs(inp['rg']))[0]
    k0g = torch.full_like(d['k0_cl'], PREFILL)
    ops.feat_generic_bwd_k0(d['sc'], d['p'], cu(with_sentinels(inp['sel'], cap + 8, 1), torch.uint8), skip, ld,
                            cu([cap + 50], torch.int32), cap, d['fg'], d['rg'], k0g)
    torch.cuda.synchronize()
    to_cl = lambda x: npf(x).transpose(1, 2, 3, 0)
    check('k0_grad', k0g, PREFILL + to_cl(r64['k0_grad']), PREFILL + to_cl(r32['k0_grad']), PREFILL + to_cl(contrib['k0_grad']),
          ulps=16)


def test_generic_k0_backward_ignores_unselected_rows_and_an_empty_count():
    from poseprobe_amd import ops
    case, M = FEAT_CASES[1], 64
    C, skip, Lp, Lv, ld, _, _ = case
    inp = feat_inputs(M, case, seed=1)
    d = feat_device(inp, case, M)
    k0g = torch.full_like(d['k0_cl'], PREFILL)
    ops.feat_generic_bwd_k0(d['sc'], d['p'], torch.zeros(M, dtype=torch.uint8, device='cuda'), skip, ld, cu([M], torch.int32), M,
                            d['fg'], d['rg'], k0g)
    ops.feat_generic_bwd_k0(d['sc'], d['p'], None, skip, ld, cu([0], torch.int32), M, d['fg'], d['rg'], k0g)
    feat = cu(np.full((M, ld), SENT, np.float32))
    ops.feat_generic_fwd(d['sc'], d['k0_cl'], d['p'], d['vd'], d['rid'], None, None, None, skip, ld, cu([0], torch.int32), M, feat, None)
    torch.cuda.synchronize()
    assert (k0g == PREFILL).all()
    assert_untouched('feat (count 0)', feat, 0)


@pytest.mark.parametrize('skip,ld', [(13, 96), (-1, 96), (3, 80), (3, 64)])
def test_generic_k0_backward_refuses_bad_arguments_without_a_launch(skip, ld):
    """As the forward: k0_skip outside 0..k0_dim, ld no multiple of 32, a feature width beyond ld (69 > 64)."""
    from poseprobe_amd import ops, _lib
    case, M = FEAT_CASES[1], 16
    inp = feat_inputs(M, case, seed=1)
    d = feat_device(inp, case, M)
    k0g = torch.full_like(d['k0_cl'], PREFILL)
    feat = cu(np.full((M, 96), SENT, np.float32))
    with pytest.raises(_lib.PoseProbeError):
        ops.feat_generic_bwd_k0(d['sc'], d['p'], None, skip, ld, cu([M], torch.int32), M, d['fg'], d['rg'], k0g)
    with pytest.raises(_lib.PoseProbeError):
        ops.feat_generic_fwd(d['sc'], d['k0_cl'], d['p'], d['vd'], d['rid'], None, None, None, skip, ld, cu([M], torch.int32), M,
                             feat, None)
    torch.cuda.synchronize()
    assert (k0g == PREFILL).all() and (feat == SENT).all()


# ------------------------------------------------------------------------------------------------------------------ MLP
MLP_SHAPES = [(7, 32, 1), (72, 96, 2), (128, 128, 4), (40, 64, 8)]
ALL_SIZES = [(0, 40), (1, 1), (63, 63), (64, 64), (65, 130), (1000, 1003)]
MLP_CASES = ([((72, 96, 2), s, None) for s in ALL_SIZES] + [(sh, s, None) for sh in MLP_SHAPES if sh != (72, 96, 2) for s in ALL_SIZES[4:]]
             + [((61, 64, 3), s, dict(mlp_fused=0)) for s in ALL_SIZES[4:]])
VALUE_TOL = dict(rtol=1e-4, atol=1e-5)                       # tests/test_hip_mlp.py, rgbnet chain
GRAD_TOL = dict(rtol=1e-3, atol=2e-5, scaled=1e-3)


@functools.lru_cache(maxsize=None)
def mlp_case(width, n_gemm, M, la_ld):
    """Inputs and the float64 reference of one MLP case, computed once and shared by every route that runs it."""
    layers, feat = GR.mlp_inputs(width, n_gemm, M, seed=5)
    g = torch.Generator().manual_seed(M + 2)
    og = torch.randn(M, 3, generator=g)
    la = torch.randn(M, la_ld, generator=g) if la_ld else None
    return dict(layers=layers, feat=feat, og=og, la=la, r64=GR.mlp(layers, feat, la, out_grad=og) if M else None)


def pack_params(layers, in_ld):
    W0 = torch.zeros(128, in_ld)
    W0[:, :layers[0][0].shape[1]] = layers[0][0]
    return torch.cat([W0.reshape(-1), layers[0][1]] + [t.reshape(-1) for W, b in layers[1:] for t in (W, b)])


def unpack_params(flat, in_ld, n_gemm):
    out, o = [], 0
    for rows, cols in [(128, in_ld)] + [(128, 128)] * (n_gemm - 1) + [(3, 128)]:
        out.append((flat[o:o + rows * cols].reshape(rows, cols), flat[o + rows * cols:o + rows * cols + rows]))
        o += rows * cols + rows
    return out, o


def guarded(floats, fill):
    t = torch.full((floats + GUARD,), fill, device='cuda')
    t[floats:] = SENT
    return t


def run_mlp(shape, M, cap, la_ld, ctx=None, want_feat_grad=True, forward_only=False):
    """pp_mlp_fwd and pp_mlp_bwd with sentinel rows past M, NaN-filled workspaces of the library's own sizes followed by a
    sentinel guard, and pre-filled (accumulating) parameter gradients."""
    from poseprobe_amd import ops
    width, in_ld, n_gemm = shape
    c = mlp_case(width, n_gemm, M, la_ld)
    P = pack_params(c['layers'], in_ld)
    params = torch.zeros(P.numel() + 60, device='cuda')
    params[:P.numel()] = P.cuda()
    feat = torch.full((cap, in_ld), SENT)
    feat[:M] = 0
    feat[:M, :width] = c['feat']
    og = torch.full((cap, 3), SENT)
    og[:M] = c['og']
    la = lg = None
    if la_ld:
        la = torch.full((cap, la_ld), SENT)
        la[:M] = c['la']
        la, lg = la.cuda(), torch.full((cap, la_ld), SENT, device='cuda')
    a_floats, s_floats = ops.mlp_workspace(in_ld, n_gemm, cap)
    assert a_floats == n_gemm * cap * 128 and s_floats >= 2 * cap * 128 + 128 * 128
    acts, scratch = guarded(a_floats, float('nan')), guarded(s_floats, float('nan'))
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    out = torch.full((cap, 3), SENT, device='cuda')
    feat, og = feat.cuda(), og.cuda()
    ops.mlp_fwd(params, feat, in_ld, n_gemm, count, cap, la, la_ld, None if forward_only else acts, out, ctx)
    res = dict(out=out, case=c, acts=acts, a_floats=a_floats)
    if not forward_only:
        pgrad = torch.full_like(params, PREFILL)
        fgrad = torch.full((cap, in_ld), SENT, device='cuda') if want_feat_grad else None
        ops.mlp_bwd(params, feat, in_ld, n_gemm, acts, out, og, count, cap, scratch, pgrad, fgrad, lg, la_ld, ctx)
        res.update(pgrad=pgrad, fgrad=fgrad, lgrad=lg, scratch=scratch, s_floats=s_floats, n_params=P.numel(), og=og)
    torch.cuda.synchronize()
    return res


def check_mlp(res, shape, M, la_ld, name=''):
    width, in_ld, n_gemm = shape
    r64 = res['case']['r64']
    assert (res['acts'][res['a_floats']:] == SENT).all(), 'acts: the guard behind the workspace was written'
    assert (res['scratch'][res['s_floats']:] == SENT).all(), 'scratch: the guard behind the workspace was written'
    assert_untouched('out', res['out'], M)
    if res['fgrad'] is not None:
        assert_untouched('feat_grad', res['fgrad'], M)
    if la_ld:
        assert_untouched('logit_add_grad', res['lgrad'], M)
        assert (res['lgrad'][:, 3:] == SENT).all(), 'only the first three columns of logit_add_grad are written'
    pg = res['pgrad'].cpu()
    assert (pg[res['n_params']:] == PREFILL).all()
    if M == 0:
        assert (pg == PREFILL).all(), 'an empty count adds nothing to the parameter gradients'
        return
    c = lambda t: t.detach().cpu().double().numpy()
    assert_close(c(res['out'][:M]), c(r64['out']), name=name + 'rgb', **VALUE_TOL)
    if res['fgrad'] is not None:
        assert_close(c(res['fgrad'][:M, :width]), c(r64['feat_grad']), name=name + 'feat_grad', **GRAD_TOL)
        assert (res['fgrad'][:M, width:] == 0).all(), 'zero weight columns pass no gradient to the padding features'
    if la_ld:
        assert_close(c(res['lgrad'][:M, :3]), c(r64['logit_grad']), name=name + 'logit_add_grad', **GRAD_TOL)
    got, used = unpack_params(pg, in_ld, n_gemm)
    assert used == res['n_params']
    for i, ((gW, gb), (rW, rb)) in enumerate(zip(got, r64['params_grad'])):
        if i == 0:
            assert (gW[:, width:] == PREFILL).all(), 'zero feature columns leave the padding of W0 without a gradient'
            gW = gW[:, :width]
        assert_close(c(gW) - PREFILL, c(rW), name=f'{name}W{i} grad', **GRAD_TOL)
        assert_close(c(gb) - PREFILL, c(rb), name=f'{name}b{i} grad', **GRAD_TOL)


@pytest.mark.parametrize('la_ld', [0, 4, 12])
@pytest.mark.parametrize('shape,size,options', MLP_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else None)
def test_layered_mlp_fwd_bwd_match_float64_autograd(shape, size, options, la_ld):
    """Every in_ld the entry points accept, 1 to 8 hidden layers (pp_mlp_workspace's n_gemm > 3 branch included), with and
    without logit_add, row counts around the 64-row tile; the 64 / 3 shape layer by layer under option mlp_fused = 0."""
    from poseprobe_amd import ops
    M, cap = size
    ctx = ops.Context(**options) if options else None
    res = run_mlp(shape, M, cap, la_ld, ctx)
    check_mlp(res, shape, M, la_ld)


def test_layered_mlp_backward_without_a_feature_gradient():
    shape, (M, cap) = (72, 96, 2), (65, 130)
    res = run_mlp(shape, M, cap, 4, want_feat_grad=False)
    check_mlp(res, shape, M, 4)


# ------------------------------------------------------------------------------------------------------------------ diffuse logits
LOGIT_SHAPE = (61, 64, 3)
ROUTES = {'layered': dict(mlp_fused=0), 'fp32_fused': dict(mlp_split=0), 'split_fused': {}}
LOGIT_CASES = ([(r, s) for r in ROUTES for s in [(1, 1), (63, 63), (64, 64), (65, 130)]]
               + [(r, (2053, 2060)) for r in ('fp32_fused', 'split_fused')])


def route_context(route, M):
    """The route's options; at 2053 rows with 16 work-groups, so that each of them owns at least two of the 33 tiles and the fused
    backward kernels stage the next tile's logit gradients while the current tile computes."""
    from poseprobe_amd import ops
    options = dict(ROUTES[route], **({'mlp_wgs': 16} if M > 2000 else {}))
    return ops.Context(**options) if options else None


def check_logit_grad_formula(res, M):
    """logit_add_grad = rgb_grad * rgb * (1 - rgb) of the route's own rgb, to 4 float32 ulps."""
    rgb, og = npf(res['out'][:M]), npf(res['og'][:M])
    want = og * rgb * (1 - rgb)
    err = np.abs(npf(res['lgrad'][:M, :3]) - want)
    assert (err <= 4 * EPS * np.abs(want) + 1e-37).all(), f'logit_add_grad: {err.max():.3e} from rgb_grad rgb (1 - rgb)'


@pytest.mark.parametrize('route,size', LOGIT_CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_diffuse_logits_on_each_route_match_float64_autograd(route, size):
    M, cap = size
    res = run_mlp(LOGIT_SHAPE, M, cap, 4, route_context(route, M))
    check_mlp(res, LOGIT_SHAPE, M, 4, name=route + ' ')
    check_logit_grad_formula(res, M)


def test_diffuse_logits_split_precision_route_is_as_accurate_as_the_fp32_route():
    """The rule of tests/test_hip_mlp.py: against float64 the RMS error of the default (split-precision) route is at most 1.25 x that of
    the fp32-instruction route (mlp_split = 0), plus 1e-12 - for rgb, logit_add_grad and feat_grad at the size where an RMS over
    thousands of entries means something (2053 rows, 16 work-groups)."""
    M, cap = 2053, 2060
    r64 = mlp_case(61, 3, M, 4)['r64']
    rms = {}
    for route in ('fp32_fused', 'split_fused'):
        res = run_mlp(LOGIT_SHAPE, M, cap, 4, route_context(route, M))
        e = lambda a, b: float(np.sqrt(((npf(a) - npf(b)) ** 2).mean()))
        rms[route] = dict(rgb=e(res['out'][:M], r64['out']), logit_add_grad=e(res['lgrad'][:M, :3], r64['logit_grad']),
                          feat_grad=e(res['fgrad'][:M, :61], r64['feat_grad']))
    print('rms errors against float64:', rms)
    for k, a in rms['fp32_fused'].items():
        b = rms['split_fused'][k]
        assert b <= 1.25 * a + 1e-12, f'{k}: fp32 instructions {a:.3e}, split precision {b:.3e}'


def test_diffuse_logits_forward_only_gives_the_same_bits():
    """acts = NULL (inference) with logit_add on the default route."""
    M, cap = 2053, 2060
    a = run_mlp(LOGIT_SHAPE, M, cap, 4, route_context('split_fused', M))
    b = run_mlp(LOGIT_SHAPE, M, cap, 4, route_context('split_fused', M), forward_only=True)
    assert torch.equal(a['out'], b['out'])
    assert_untouched('out', b['out'], M)
    assert_close(npf(b['out'][:M]), npf(a['case']['r64']['out']), name='forward-only rgb', **VALUE_TOL)
