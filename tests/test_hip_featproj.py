"""Surface-projection feature pass (TrainEngine.surface_projection_grads, csrc/pp_featproj.hip): parity with the reference's
recorded get_project_feature_loss, the parameter gradients against autograd through the drop-in module, the loss kernels alone
against the float64 restatement on constructed inputs, bit reproducibility, a buffer fence, and the joint step."""
import functools

import numpy as np
import pytest
import torch

from tests import featproj_reference as R
from tests.helpers import assert_close, load

pytestmark = pytest.mark.gpu

GS = R.GS
RK = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, flip_x=False, flip_y=False)
CASE = 'featproj_g24'


@functools.lru_cache(maxsize=None)
def _fixture():
    return load('featproj_g24.npz'), R.fixture_params(), R.feature_maps(CASE, R.NV, R.LAYERS)


def _engine(featproj_rows=R.ROWS, n_rand=64, maps=True, **kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    d, P, feats = _fixture()
    rs = syn.range_shape()
    H, W = int(d['H']), int(d['W'])
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, int(d['G']) ** 3, out_range=float(rs.max()))
    eng = TrainEngine(cfg, 3, H, W, n_rand, featproj_rows=featproj_rows, **kw)
    eng.set_views(np.zeros((3, H, W, 3), np.float32), np.ones((3, H, W, 1), np.float32), d['Ks'], d['w2c_init'])
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'], se3=torch.tensor(d['se3']))
    if maps and featproj_rows:
        eng.set_feature_maps(feats)
    eng.zero_grads()
    return eng


def _rows(dev='cuda'):
    """The recorded draw: pixels of view 0 through their centres (the reference's flattened training rays are row-major)."""
    d = _fixture()[0]
    idx, W = torch.tensor(d['pix_index']), int(d['W'])
    pix = torch.stack([(idx % W).float() + 0.5, (idx // W).float() + 0.5], -1)
    i, j = (int(v) for v in d['pair'])
    return dict(src=torch.zeros(idx.shape[0], dtype=torch.int32, device=dev), pix=pix.to(dev).contiguous(), own=i, other=j)


def _main_pass(eng):
    """The step's own pass (pose, BARF weights), then clean gradient buffers: what is left afterwards is the pass's share."""
    g = torch.Generator().manual_seed(0)
    ray_idx = torch.randperm(3 * eng.H * eng.W, generator=g)[:eng.N].to(torch.int32).cuda()
    eng.render_and_grads(ray_idx, torch.rand(eng.N, generator=g).cuda(), GS)
    eng.zero_grads()


def _pass_kw():
    d = _fixture()[0]
    return dict(weight=1.0, nl=float(d['nl']), jitter=torch.tensor(d['jitter']).cuda(), jitter_ref=torch.tensor(d['jitter_ref']).cuda(),
                scale=1.0)


@pytest.mark.parametrize('featproj_rows', [96, 104])
def test_pass_matches_the_reference(featproj_rows):
    """loss, n_valid, the exact set of valid rows and d loss / d se3 of the native pass == what the reference's
    get_project_feature_loss produced (fixture), with the tolerances of test_hip_reproj.test_pass_matches_the_reference.
    featproj_rows = 104: the fixture's 96 rows on a larger capacity - eight rays that miss the box go through the whole chain of
    both queries; same expectations, nothing but finite values in the gradients."""
    d = _fixture()[0]
    eng = _engine(featproj_rows)
    _main_pass(eng)
    eng.surface_projection_grads(_rows(), GS, **_pass_kw())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.flat.grad).all()) and bool(torch.isfinite(eng.se3_grad).all())
    ws, wb, fp = eng.ws_featproj, eng.ws_featproj_ref, eng._fp
    assert ws.N == wb.N == featproj_rows
    for w in (ws, wb):
        assert int(w.ray_start[96]) == int(w.ray_start[featproj_rows])                       # the padding rows have no sample
    assert_close(ws.rays_o[:96], d['a.o'], rtol=1e-5, atol=1e-6, name='rays_o of query A')
    assert_close(ws.rays_d[:96], d['a.d'], rtol=1e-5, atol=1e-6, name='rays_d of query A')
    assert_close(wb.rays_d[:96], d['b.d'], rtol=1e-4, atol=1e-4, name='rays_d of query B')
    t = eng.last_featproj_terms
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in t.values()) and t['cos'].shape == (2,)
    valid = fp['valid'].cpu().numpy().astype(bool)
    print(f"loss {float(t['loss']):.7g} (ref {float(d['loss']):.7g}) n_valid {float(t['n_valid'])} (ref {int(d['valid'].sum())})")
    print('se3 grad', eng.se3_grad.cpu().numpy(), 'ref', d['g_se3'])
    assert np.array_equal((ws.depth_acc[:96] > 0).cpu().numpy(), d['hit']) and np.array_equal((wb.depth_acc[:96] > 0).cpu().numpy(), d['hit_ref'])
    assert np.array_equal(valid[:96], d['valid']) and not valid[96:].any()
    assert float(t['n_valid']) == float(d['valid'].sum())
    assert_close(np.float32(t['loss'].item()), d['loss'], rtol=2e-4, atol=1e-5, name='loss')
    assert_close(eng.se3_grad.cpu().numpy(), d['g_se3'], rtol=2e-3, atol=1e-4, scaled=1e-3, name='d/d se3')
    assert float(np.abs(d['g_se3']).max()) > 1e-3 and float(eng.se3_grad[0].abs().max()) == 0.0       # view 0 is not refined


def _autograd(model):
    """recon_utils.get_project_feature_loss on `model` through autograd."""
    from poseprobe_amd import camera
    from poseprobe_amd import recon_utils as RU
    d, _, feats = _fixture()
    dev = 'cuda'
    se3 = torch.tensor(d['se3'], device=dev, requires_grad=True)
    init = torch.tensor(d['w2c_init'], device=dev)
    w2c = torch.cat([init[:1], camera.pose.compose([camera.lie.se3_to_SE3(se3), init])[1:]], 0)
    rows, kw = _rows(), _pass_kw()
    loss = RU.get_project_feature_loss(model, torch.tensor(d['Ks'], device=dev), np.array([[int(d['H']), int(d['W'])]] * 3), kw['nl'], GS,
                                       w2c, [f.to(dev) for f in feats], rows['src'].long(), rows['pix'], rows['own'], rows['other'],
                                       jitter=kw['jitter'], jitter_ref=kw['jitter_ref'], **RK)
    return loss, se3


def test_gradients_reach_the_warp_network_alpha_beta_and_the_poses():
    """flat.grad and se3_grad of the pass == autograd of recon_utils.get_project_feature_loss on engine.voxurf_view(), at the
    tolerances of test_hip_reproj.test_render_mode_reaches_the_warp_network_and_alpha_beta; the colour grid's gradient and its
    touch marks stay exactly as they were."""
    from poseprobe_amd import recon_utils as RU
    d = _fixture()[0]
    eng = _engine()
    _main_pass(eng)
    g = torch.Generator().manual_seed(1)
    eng.k0_grad.copy_(torch.randn(eng.k0_grad.shape, generator=g))
    eng.k0_touched.copy_(torch.randint(0, 2, eng.k0_touched.shape, generator=g).to(torch.uint8))
    k0_grad, touched = eng.k0_grad.clone(), eng.k0_touched.clone()
    eng.surface_projection_grads(_rows(), GS, **_pass_kw())
    torch.cuda.synchronize()
    assert torch.equal(eng.k0_grad, k0_grad) and torch.equal(eng.k0_touched, touched)
    model = eng.voxurf_view()
    loss, se3 = _autograd(model)
    loss.backward()
    assert np.array_equal(RU.get_project_feature_loss.last_valid.cpu().numpy(), d['valid'])
    assert_close(eng.last_featproj_terms['loss'], loss.detach(), rtol=2e-4, atol=1e-5, name='loss')
    tol = dict(rtol=2e-3, atol=1e-5, scaled=1e-3)
    print('se3', eng.se3_grad.cpu().numpy(), se3.grad.cpu().numpy())
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


# ---------------------------------------------------------------------------------------------------------------------------
# the loss kernels alone, on constructed inputs
HC = WC = 33                                    # W - 1 = 32: pixel 32 is x = 1 exactly
INTR = [[32., 32., 16., 16.], [30., 34., 15.5, 16.25], [40., 40., 16., 16.]]
NL, VOXEL = 0.05, 0.04
KERNEL_CASES = ('causes', 'C1', 'C20', 'C64', 'C256', 'C512', 'zero_vector', 'none_valid')
OUTPUTS = ('loss', 'sum_cos', 'cos', 'g_depth', 'g_o', 'g_d', 'g_w2c')


def _poses():
    """View 0 at the origin looking along +z; view 1 ahead of it and to the side, turned by 0.3 rad; view 2 takes no part."""
    out = [np.concatenate([np.eye(3), np.zeros((3, 1))], 1)]
    for a, c in ((0.3, (0.4, 0.1, 1.0)), (-0.4, (-0.5, 0.0, 0.2))):
        Rm = np.array([[np.cos(a), 0., -np.sin(a)], [0., 1., 0.], [np.sin(a), 0., np.cos(a)]])
        out.append(np.concatenate([Rm, (-Rm @ np.array(c))[:, None]], 1))
    return torch.tensor(np.stack(out), dtype=torch.float32)


def _query(o, p, frac):
    """A ray from o whose surface point is p exactly where the inputs are dyadic: d = p - o, depth 1 = t_min + acc."""
    n = p.shape[0]
    t_min = torch.full((n,), frac)
    return dict(o=o.expand(n, 3).clone(), d=(p - o).clone(), t_min=t_min, acc=1.0 - t_min)


@functools.lru_cache(maxsize=None)
def _kernel_problem(case):
    """-> (qa, qb, w2c, intr, feats, n): n rows.  Rows are drawn at random in front of both cameras and kept when the float64
    decisions leave a margin of 1e-2, so float32 and float64 decide every row alike; the special rows are placed by hand."""
    C = {'causes': 20, 'zero_vector': 20, 'none_valid': 20}.get(case) or int(case[1:])
    layers = ((C, 9, 9), (max(C // 2, 3), 5, 7))               # w - 1 = 8: texel 7 of layer 0 is pixel 28 of view 0 exactly
    w2c, intr = _poses(), torch.tensor(INTR)
    g = torch.Generator().manual_seed(len(case) * 131 + C)
    cand = torch.stack([(torch.rand(400, generator=g) - 0.5) * 1.6, (torch.rand(400, generator=g) - 0.5) * 1.2,
                        1.8 + torch.rand(400, generator=g) * 1.2], -1)
    special = {
        'x_is_one': [1.0, 0.25, 2.0],                       # u = (32 + 16 * 2) / 2 = 32 in view 0: x = 1 exactly, still inside
        'texel': [0.75, 0.25, 2.0],                         # u = 28, v = 20 in view 0: texel (7, 5) of layer 0 exactly
        'zero': [0.625, -0.125, 2.0],                       # u = 26, v = 14: inside the cell (6..7, 3..4) of layer 0
    }
    p = torch.cat([torch.tensor([special['x_is_one'], special['texel'], special['zero']]), cand])
    o_a = torch.zeros(3)
    c_j = -(w2c[1, :, :3].T @ w2c[1, :, 3])
    ref_off = torch.zeros_like(p)
    ref_off[:, 0] = 0.3 * VOXEL * torch.where(torch.arange(p.shape[0]) % 2 == 0, 1.0, -1.0)
    qa, qb = _query(o_a, p, 0.5), _query(c_j, p + ref_off, 0.25)
    dec = R.decisions(qa, qb, w2c, intr, 0, 1, NL, VOXEL, HC, WC)
    margins = R.row_margins(dec, NL)
    margins[:2] = 1.0                                        # the two exact rows sit ON a decision by construction, on its inside
    ok = ~torch.stack(list(dec['reject'].values())).any(0) & (margins > 1e-2)
    assert bool(ok[:3].all()), 'a hand-placed row is not valid'
    keep = torch.nonzero(ok).flatten()
    n_keep = {'causes': 24, 'zero_vector': 12, 'none_valid': 7}.get(case, 70)
    keep = keep[:n_keep]
    assert keep.shape[0] == n_keep
    if case != 'zero_vector':
        keep = keep[keep != 2]
    sel = lambda q: {k: v[keep].clone() for k, v in q.items()}
    qa, qb = sel(qa), sel(qb)
    n = keep.shape[0]
    if case in ('causes', 'none_valid'):
        # one rejection cause per row, each row otherwise valid: rows 2.. of 'causes', every row of 'none_valid'
        first = 2 if case == 'causes' else 0
        r = first
        qa['t_min'][r], qa['acc'][r] = 1.0, 0.0                                          # query A hits nothing
        qb['t_min'][r + 1], qb['acc'][r + 1] = 1.0, 0.0                                  # query B hits nothing
        qb['d'][r + 2, 0] += 5 * VOXEL                                                   # the two surface points lie 5 voxels apart
        for row, pt in ((r + 3, [1.4, 0.1, 2.0]), (r + 4, [-0.5, 0.0, 2.0]), (r + 5, [0.3, 0.1, 0.9])):
            # outside view 0 only (u = 38.4) | outside view 1 only | behind view 1's near plane (inside view 0): q := nl, u = fx + cx
            pt = torch.tensor(pt)
            qa['d'][row] = pt - o_a
            qb['d'][row] = pt + torch.tensor([0.3 * VOXEL, 0., 0.]) - c_j
        dec = R.decisions(qa, qb, w2c, intr, 0, 1, NL, VOXEL, HC, WC)
        rej = {k: torch.nonzero(v).flatten().tolist() for k, v in dec['reject'].items()}
        assert rej == dict(miss=[r], miss_ref=[r + 1], far=[r + 2], outside_i=[r + 3], outside_j=[r + 4, r + 5]), rej
        assert bool((dec['qz'][r + 5, 1] < NL)) and int((dec['qz'] < NL).sum()) == 1
        assert float(R.row_margins(dec, NL)[2:].min()) > 1e-2
    feats = R.feature_maps('kernel/' + case, 3, layers, noise=0.2)
    if case == 'zero_vector':
        feats[0][0, :, 3:5, 6:8] = 0.0                                                   # the four taps of row 2 in view 0, every channel
    return qa, qb, w2c, intr, feats, n


def _run_kernels(case, cap_extra=5, fence=None):
    """pp_featproj_loss on the case with capacity = n + cap_extra; the padding rows of every input hold NaN."""
    from poseprobe_amd import ops
    qa, qb, w2c, intr, feats, n = _kernel_problem(case)
    cap, L = n + cap_extra, len(feats)

    def padded(t):
        out = torch.full((cap,) + tuple(t.shape[1:]), float('nan'))
        out[:n] = t
        return out.cuda().contiguous()
    A, B = {k: padded(v) for k, v in qa.items()}, {k: padded(v) for k, v in qb.items()}
    shapes = dict(terms=(6,), valid=(cap,), cos=(L, cap), g_q=(cap, 6), g_depth=(cap,), g_o=(cap, 3), g_d=(cap, 3), g_w2c=(3, 3, 4))
    if fence is None:
        out = {k: torch.full(s, float('nan'), device='cuda') for k, s in shapes.items() if k != 'valid'}
        out['valid'] = torch.full((cap,), 7, dtype=torch.uint8, device='cuda')
    else:
        out = {k: fence(k, s) for k, s in shapes.items()}
    maps = [f.permute(0, 2, 3, 1).contiguous().cuda() for f in feats]
    ops.featproj_loss(n, 0, 1, A['o'], A['d'], A['t_min'], A['acc'], B['o'], B['d'], B['t_min'], B['acc'], intr.cuda(), w2c.cuda(), NL,
                      VOXEL, HC, WC, maps, 0.7, 0.5, out['terms'], out['valid'], out['cos'], out['g_q'], out['g_depth'], out['g_o'],
                      out['g_d'], out['g_w2c'])
    torch.cuda.synchronize()
    return out, n, cap


def _restate(case, dtype):
    qa, qb, w2c, intr, feats, n = _kernel_problem(case)
    return R.restate(qa, qb, w2c, intr, 0, 1, NL, VOXEL, HC, WC, feats, weight=0.7, scale=0.5, dtype=dtype)


def _rel(a, b):
    """max |a - b| / max |b| (0 where b is all zero and a is too)."""
    a, b = a.double(), b.double()
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / scale if scale > 0 else float((a - b).abs().max())


@functools.lru_cache(maxsize=None)
def _float32_loss_of_the_restatement():
    """Per output, what the restatement itself loses in float32 against float64, as max |x32 - x64| / max |x64|: the largest over
    KERNEL_CASES but 'C1', and 'C1' on its own (-> pooled, of C1).  With one channel cos is +-1 and its derivative the difference
    of two equal terms of size 1 / |a|: float32 leaves 1e-5 of the row's other gradient there, in the restatement as in any
    kernel, and pooling that with the other cases would widen their bound twentyfold."""
    pooled, own = dict.fromkeys(OUTPUTS, 0.0), {}
    for case in KERNEL_CASES:
        r64, r32 = _restate(case, torch.float64), _restate(case, torch.float32)
        assert torch.equal(r64['valid'], r32['valid']), case
        for k in OUTPUTS:
            e = _rel(torch.as_tensor(r32[k]), torch.as_tensor(r64[k]))
            if case == 'C1':
                own[k] = e
            else:
                pooled[k] = max(pooled[k], e)
    return pooled, {k: max(pooled[k], own[k]) for k in OUTPUTS}


@pytest.mark.parametrize('case', KERNEL_CASES)
def test_loss_kernels_equal_the_float64_restatement(case):
    """pp_featproj_loss against tests/featproj_reference.restate in float64: the flags exactly, every other output within 4 x what
    the same restatement loses in float32 against float64 on these inputs (error = max |x - ref| / max |ref| per output; the loss
    is the largest over the cases, C = 1 apart: _float32_loss_of_the_restatement).  Measured float32 losses of the restatement:
    loss 8.1e-08, sum_cos 9.7e-07, cos 7.6e-07, g_depth 1.4e-06, g_o 8.1e-07, g_d 8.1e-07, g_w2c 3.6e-07; at C = 1 g_o and g_d
    1.6e-05, g_w2c 3.4e-06 (printed by every run; the host's float32 kernels move them in the first digit).  The kernels' own
    errors against float64 on the MI355X: between 0.1 and 1 x these figures, 1.8 x for g_o / g_d / g_w2c at C = 1.
    Cases: 'causes' - every rejection cause in a row of its own (query A misses, query B misses, surface points 5 voxels apart,
    outside view i only, outside view j only, behind view j's near plane), a projection exactly on x = 1 and one exactly on a
    texel; C = 1, 20, 64, 256, 512 (scalar and 16-byte loads, one and two rounds of the lanes); a zero feature vector (the eps
    rule and its derivative); no valid row (everything exactly 0).  Always n_rows < capacity: the padding rows of every input
    hold NaN and must leave zeros."""
    budget = _float32_loss_of_the_restatement()[case == 'C1']
    ref = _restate(case, torch.float64)
    out, n, cap = _run_kernels(case)
    L = ref['cos'].shape[0]
    print(case, 'float32 loss of the restatement', {k: f'{v:.2e}' for k, v in budget.items()})
    for k, t in out.items():
        assert bool(torch.isfinite(t.float()).all()), f'{case} {k}'
    valid = out['valid'].cpu().bool()
    assert torch.equal(valid[:n], ref['valid']) and not bool(valid[n:].any())
    assert float(out['terms'][1]) == float(ref['n_valid'])
    for k in ('g_q', 'g_depth', 'g_o', 'g_d'):
        assert float(out[k][n:].abs().max()) == 0.0 and float(out[k][:n][~valid[:n].cuda()].abs().sum()) == 0.0, f'{case} {k}'
    assert float(out['cos'][:, n:].abs().max()) == 0.0 and float(out['terms'][2 + L:].abs().sum()) == 0.0
    got = dict(loss=out['terms'][0].cpu(), sum_cos=out['terms'][2:2 + L].cpu(), cos=out['cos'][:, :n].cpu(), g_depth=out['g_depth'][:n].cpu(),
               g_o=out['g_o'][:n].cpu(), g_d=out['g_d'][:n].cpu(), g_w2c=out['g_w2c'].cpu())
    if case == 'none_valid':
        assert ref['n_valid'] == 0
        for k, t in got.items():
            assert float(t.abs().max()) == 0.0, k
        return
    assert ref['n_valid'] >= 5
    errs = {k: _rel(got[k], torch.as_tensor(ref[k])) for k in OUTPUTS}
    print(case, 'kernel against float64', {k: f'{v:.2e}' for k, v in errs.items()})
    for k in OUTPUTS:
        assert errs[k] <= 4 * budget[k], f'{case} {k}: {errs[k]:.3e} > 4 x {budget[k]:.3e}'
    assert float(got['g_w2c'][2].abs().max()) == 0.0 and float(got['g_w2c'][:2].abs().max()) > 0
    if case == 'zero_vector':
        # |a| = 0 in layer 0 of row 2: cos = 0 / (eps |b|) = 0 exactly, nothing of 0 / 0; the layer's gradient vanishes with the taps
        # (d a / d position = 0, d cos / d b = a / .. = 0), the other layer's share of the row is there
        assert float(got['cos'][0, 2]) == 0.0 and float(ref['cos'][0, 2]) == 0.0 and float(got['g_o'][2].abs().max()) > 0


def test_reprojection_kernel_equals_the_restatement():
    """pp_featproj_reproject == step 2 in float64 (the pixel, rtol 1e-5), the near-plane row included; padding rows get view -1."""
    from poseprobe_amd import ops
    qa, _, w2c, intr, _, n = _kernel_problem('causes')
    cap = n + 3
    pad = lambda t: torch.cat([t, torch.full((3,) + tuple(t.shape[1:]), float('nan'))]).cuda().contiguous()
    own, pix = torch.full((cap,), 9, dtype=torch.int32, device='cuda'), torch.full((cap, 2), float('nan'), device='cuda')
    ops.featproj_reproject(n, 1, pad(qa['o']), pad(qa['d']), pad(qa['t_min']), pad(qa['acc']), intr.cuda(), w2c.cuda(), NL, own, pix)
    ref = R.reproject(qa['o'], qa['d'], qa['t_min'], qa['acc'], w2c, intr, 1, NL)
    assert own.tolist() == [1] * n + [-1] * 3 and float(pix[n:].abs().max()) == 0.0
    assert_close(pix[:n], ref, rtol=1e-5, atol=1e-5, name='pix_ref')
    assert_close(pix[7], torch.tensor([30. + 15.5, 34. + 16.25]), rtol=1e-6, atol=0, name='behind the near plane: K (nl, nl, nl) / nl')


def test_same_inputs_give_the_same_bits():
    a, b = _run_kernels('C256')[0], _run_kernels('C256')[0]
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert float(a['g_w2c'].abs().max()) > 0


def test_new_kernels_stay_inside_their_buffers():
    """Every output of the new kernels sits in a 64 KB-sentineled arena, at C = 1, 20 and 512 (capacity = rows + 5).  Run once per
    case, no repetition."""
    from poseprobe_amd import ops
    PAD, SENT = 16384, 0x7FC0DEAD
    for case in ('C1', 'causes', 'C512'):
        fences = {}

        def fenced(name, shape, dtype=torch.float32):
            n = int(np.prod(shape))
            if name == 'valid':
                arena = torch.full((n + 2 * PAD,), 0xA5, dtype=torch.uint8, device='cuda')
            else:
                arena = torch.empty(n + 2 * PAD, dtype=torch.int32, device='cuda').fill_(SENT).view(dtype)
            fences[name] = (arena, n)
            return arena[PAD:PAD + n].view(*shape)
        out, n, cap = _run_kernels(case, fence=fenced)
        qa, _, w2c, intr, _, _ = _kernel_problem(case)
        own = fenced('own_ref', (cap,), torch.int32)
        pix = fenced('pix_ref', (cap, 2))
        q = {k: torch.cat([v, v.new_zeros((5,) + tuple(v.shape[1:]))]).cuda() for k, v in qa.items()}
        ops.featproj_reproject(n, 1, q['o'], q['d'], q['t_min'], q['acc'], intr.cuda(), w2c.cuda(), NL, own, pix)
        torch.cuda.synchronize()
        for name, (arena, m) in fences.items():
            if name == 'valid':
                assert bool((arena[:PAD] == 0xA5).all()) and bool((arena[PAD + m:] == 0xA5).all()), f'{case} {name}'
                assert bool((arena[PAD:PAD + m] <= 1).all())
            else:
                a = arena.view(torch.int32)
                assert bool((a[:PAD] == SENT).all()) and bool((a[PAD + m:] == SENT).all()), f'{case} {name}'
                assert name == 'own_ref' or bool(torch.isfinite(arena[PAD:PAD + m]).all()), f'{case} {name}'


# ---------------------------------------------------------------------------------------------------------------------------
def _joint(opt, **kw):
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.joint import DualBranchEngine
    torch.manual_seed(5)
    net = bg_nerf.NeRF(opt, device='cuda')
    net.progress.data.fill_(0.6)
    det = kw.get('deterministic', False)
    eng = _engine(**kw)
    return eng, DualBranchEngine(eng, net, depth_range=(0.5, 3.0), deterministic=det)


def _joint_batch():
    g = torch.Generator().manual_seed(3)
    V, N, S, H, W = 3, 24, 16, R.H, R.W
    ray_idx = torch.randperm(V * H * W, generator=g)[:64].to(torch.int32).cuda()
    jitter = torch.rand(64, generator=g).cuda()
    pixels = (torch.rand(N, 2, generator=g) * torch.tensor([W - 1., H - 1.])).cuda()
    image, rand = torch.rand(V, N, 3, generator=g).cuda(), torch.rand(V, N, S, 1, generator=g).cuda()
    return ray_idx, jitter, pixels, image, rand


def _state(eng, joint):
    out = dict(k0=eng.k0_cl, k0_m=eng.k0_m, k0_v=eng.k0_v, flat=eng.flat.data, flat_m=eng.flat.m, flat_v=eng.flat.v, se3=eng.se3,
               se3_m=eng.se3_m, se3_v=eng.se3_v)
    out.update({f'scene{i}': st.net.flat for i, st in enumerate(joint.scene.states)})
    return {k: v.detach().clone() for k, v in out.items()}


def test_joint_step_is_the_pass_between_the_backward_and_the_optimiser():
    """train_step(featproj=...) == render_and_grads, the scene branch, the pass, both optimisers - run by hand through
    forward_backward without the keyword and surface_projection_grads at the engine's loss_scale.  The two runs end in float
    atomics (object and scene weight gradients), whose order moves a sum by a few ulp; Adam's first step turns a gradient g into
    lr g / (|g| + 1e-8), which such noise moves by far less than 1e-3 lr wherever |g| is above the noise: every parameter within
    1e-3 of its learning rate (k0 0.1, flat and poses 1e-3); the first moments (0.1 x the gradient) at the tolerance
    test_hip_reproj compares gradients across runs with.  The weight (50: the caller's choice) makes the term's share of the
    small parameters' gradient large enough for that comparison to tell its absence: against the step without the term the moments
    differ by more than ten times the tolerance."""
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(sample_intvs=16)
    ray_idx, jitter, pixels, image, rand = _joint_batch()
    kw = _pass_kw()
    fp = dict(rows=_rows(), weight=50., nl=kw['nl'], jitter=kw['jitter'], jitter_ref=kw['jitter_ref'])
    e1, j1 = _joint(opt)
    j1.train_step(ray_idx, jitter, GS, pixels, image, depth_rand=rand, featproj=fp)
    e2, j2 = _joint(opt)
    j2.forward_backward(ray_idx, jitter, GS, pixels, image, depth_rand=rand)
    before = e2.se3_grad.clone()
    e2.surface_projection_grads(fp['rows'], GS, fp['weight'], fp['nl'], jitter=fp['jitter'], jitter_ref=fp['jitter_ref'])
    assert float((e2.se3_grad - before).abs().max()) > 0
    for k in ('loss', 'n_valid', 'cos'):
        assert torch.equal(e1.last_featproj_terms[k], e2.last_featproj_terms[k]), k
    e2.optimizer_step(True, grad_scale=1.0)
    j2.scene.optimizer_step(grad_scale=1.0)
    e3, j3 = _joint(opt)
    j3.train_step(ray_idx, jitter, GS, pixels, image, depth_rand=rand)
    torch.cuda.synchronize()
    s1, s2, s3 = _state(e1, j1), _state(e2, j2), _state(e3, j3)
    lr = lambda k: 0.1 if k.startswith('k0') else 1e-3
    for k in ('k0', 'flat', 'se3', 'scene0'):
        dev = float((s1[k] - s2[k]).abs().max())
        print(k, 'max deviation', dev)
        assert dev <= 1e-3 * lr(k), k
    # Adam's first step has the size of the learning rate whatever the gradient's: the term shows in the first moments (0.1 g)
    for k in ('se3_m', 'flat_m'):
        assert_close(s1[k], s2[k], rtol=1e-4, atol=0, scaled=1e-5, name=k)
        tol = 1e-4 * s2[k].abs() + 1e-5 * s2[k].abs().max()
        assert bool(((s1[k] - s3[k]).abs() > 10 * tol).any()), k                     # the comparison above can tell the term's absence


def test_without_the_keyword_the_step_is_bit_for_bit_the_step_of_an_engine_without_the_capacity():
    """featproj_rows > 0 with maps loaded, train_step without featproj=: every engine tensor equals, under torch.equal, the same
    step of an engine built with featproj_rows = 0.  Both engines are deterministic=True (the object and the scene branch), the
    only configuration in which two runs of a step promise equal bits at all."""
    from poseprobe_amd import bg_nerf
    opt = bg_nerf.default_options(sample_intvs=16)
    ray_idx, jitter, pixels, image, rand = _joint_batch()
    states = []
    for rows in (0, R.ROWS):
        eng, joint = _joint(opt, featproj_rows=rows, deterministic=True)
        assert (eng.ws_featproj is None) == (rows == 0)
        for step in range(2):
            joint.train_step(ray_idx, jitter, GS + step, pixels, image, depth_rand=rand)
        torch.cuda.synchronize()
        assert eng.last_featproj_terms is None
        states.append(_state(eng, joint))
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), k


def test_trainer_steps_with_the_term_and_leaves_the_scalars_on_the_device():
    """DualBranchTrainer(surface_projection=...): steps run, move the pose, and leave the scalars on the device; beyond the pose
    phase the term is off."""
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.trainer import DualBranchTrainer
    d, _, feats = _fixture()
    opt = bg_nerf.default_options(sample_intvs=16)
    opt.nerf.rand_rays = 48
    eng = _engine(featproj_rows=64, maps=False)
    tr = DualBranchTrainer(eng, opt, max_iter=10, surface_projection=dict(features=feats, pairs=[(0, 1), (1, 2)], weight=1e-3,
                                                                          nl=float(d['nl']), n_rays=64))
    for step in range(4):
        before = eng.se3.clone()
        tr.train_step(step)
        if step < 3:                                                       # pose_phase: step < 10 * 0.3
            assert tr.last_featproj['n_rows'] == 64 and tr.last_featproj['pair'] in ((0, 1), (1, 2))
            t = eng.last_featproj_terms
            assert all(v.is_cuda for v in t.values()) and float(t['n_valid']) >= 0
            assert not torch.equal(before, eng.se3)
        else:
            assert tr.last_featproj is None
        assert bool(torch.isfinite(eng.se3).all()) and bool(torch.isfinite(eng.flat.data).all())


RENDER_CALLS = ['pp_reproj_rays', 'pp_sample_dense', 'pp_mlp_pack', 'pp_warp_lean_begin', 'pp_warp_fwd', 'pp_geometry_fwd',
                'pp_color_feat_fwd', 'pp_rgbnet_fwd', 'pp_march_fwd', 'pp_reproj_loss', 'pp_march_bwd', 'pp_rgbnet_bwd',
                'pp_color_feat_bwd', 'pp_geometry_bwd', 'pp_warp_bwd', 'pp_raygen_select_bwd', 'pp_mlp_pack_invalidate',
                'pp_warp_lean_end', 'pp_reproj_pose_fold', 'pp_pose_bwd']
CROSSING_CALLS = ['pp_reproj_rays', 'pp_sample_dense', 'pp_reproj_dense_pts', 'pp_grid_sample_fwd', 'pp_sdf_first_crossing',
                  'pp_reproj_loss', 'pp_sdf_crossing_dense_bwd', 'pp_reproj_pose_fold', 'pp_pose_bwd']
FEATPROJ_CALLS = ['pp_reproj_rays', 'pp_sample_dense', 'pp_mlp_pack', 'pp_warp_lean_begin', 'pp_warp_fwd', 'pp_geometry_fwd',
                  'pp_color_feat_fwd', 'pp_rgbnet_fwd', 'pp_march_fwd', 'pp_featproj_reproject', 'pp_reproj_rays', 'pp_sample_dense',
                  'pp_warp_fwd', 'pp_geometry_fwd', 'pp_color_feat_fwd', 'pp_rgbnet_fwd', 'pp_march_fwd', 'pp_featproj_loss',
                  'pp_march_bwd', 'pp_rgbnet_bwd', 'pp_color_feat_bwd', 'pp_geometry_bwd', 'pp_warp_bwd', 'pp_raygen_select_bwd',
                  'pp_mlp_pack_invalidate', 'pp_warp_lean_end', 'pp_reproj_pose_fold', 'pp_pose_bwd']


def test_the_auxiliary_passes_make_their_library_calls_in_a_fixed_order(monkeypatch):
    """Entry points recorded around _lib.call (as tests/test_hip_step_launches.py records them) over reprojection_grads in both modes
    and surface_projection_grads, on the two 24^3 fixtures: each pass makes exactly the calls of its list, in that order - the
    weight pack and the lean scope of its own opened before the forward chain and closed behind the ray backward, ahead of the pose
    fold.  The passes share their skeleton on the host (TrainEngine._depth_loss_pass, _pose_fold); the literal lists are what a change
    to that host code may not move."""
    from poseprobe_amd import _lib
    from tests import test_hip_reproj as RP
    d = load('reproj_g24.npz')
    rp, fp = RP._engine(d), _engine()
    RP._main_pass(rp)
    _main_pass(fp)
    rows, kw = RP._rows(d), dict(jitter=torch.tensor(d['jitter']).cuda(), nl=float(d['nl']), pixel_thre=200, scale=1.0)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    seen = {}
    for mode in ('render', 'crossing'):
        names.clear()
        rp.reprojection_grads(rows, mode, GS, **kw)
        seen[mode] = list(names)
    names.clear()
    fp.surface_projection_grads(_rows(), GS, **_pass_kw())
    seen['featproj'] = list(names)
    torch.cuda.synchronize()
    for k, v in seen.items():
        print(k, v)
    assert seen['render'] == RENDER_CALLS
    assert seen['crossing'] == CROSSING_CALLS
    assert seen['featproj'] == FEATPROJ_CALLS
