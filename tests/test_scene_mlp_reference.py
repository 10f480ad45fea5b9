"""CPU checks of what tests/test_hip_scene_mlp_kernels.py rests on (tests/scene_mlp_reference.py, tests/scene_mlp_cases.py):
  * the restated layouts end where pp_nerf_workspace / pp_nerf_layout end;
  * the float64 stage references, chained, ARE oracle.scene_nerf.mlp and its autograd gradients (1e-12), on the masks the chain chose;
  * a float32 numpy pass in a third association (scene_mlp_reference.emulate32) passes helpers.check at the default 8 ulps on every
    stage; the ulps it needs are printed - the CPU half of the table in DESIGN.md, section 5;
  * the planted settings have the properties the GPU tests rest on (raw on both sides of 20, closed bands, ray lengths)."""
import numpy as np
import pytest
import torch

from oracle import scene_nerf as SN
from tests import scene_mlp_cases as C
from tests import scene_mlp_reference as MR
from tests.helpers import check, nerf_workspace_of_the_parent

F64 = torch.float64


def test_layout_walks_end_at_the_library_totals():
    from poseprobe_amd import ops
    assert MR.param_offsets() == ops.nerf_layout()
    for R, S in C.SHAPES + (C.second_tile_shape(256), C.second_strip_shape(), (1023, 128), (3072, 128)):
        M = R * S
        assert MR.workspace_floats(M, R) == ops.nerf_workspace(M, R) == nerf_workspace_of_the_parent(M, R), (M, R)


def test_mask_plane_layouts_invert_each_other():
    g = torch.Generator().manual_seed(1)
    for M in (3, 129, 257):
        st = torch.rand(M, 256, generator=g) > 0.5
        words = MR.mask_pack_cols(st)
        b = ((words + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)
        assert torch.equal(MR.mask_states_cols(b, M), st)


def test_case_settings_have_the_planted_properties():
    assert (C.band_weights(C.PROGRESS['open']) == 1).all() and (C.band_weights(C.PROGRESS['closed']) == 0).all()
    w = C.band_weights(C.PROGRESS['partly'])
    assert (w[:10] == 0).sum() == 4 and (w[:10] == 1).sum() == 5 and 0 < w[5] < 1
    assert {p for p, _ in C.SETTINGS} == set(C.PROGRESS) and {b for _, b in C.SETTINGS} == set(C.BD)
    for (R, S), (progress, bd) in zip(C.SHAPES, C.SETTINGS):
        c = C.case(R, S, progress, bd)
        n = np.linalg.norm(c['ray'], axis=1)
        assert abs(n[0] - 1e-3) < 1e-8 and (R == 1 or abs(n[-1] - 10) < 1e-5)
        raw = MR.emulate32(c, forward_only=True).A['raw']
        if bd == 20.0:
            assert min(int((raw > 20).sum()), int((raw <= 20).sum())) >= C.MIN_PER_SIDE, f'{R}x{S}: raw on both sides of 20'
        if bd == -30.0:
            assert bool((raw < -20).all()), f'{R}x{S}: raw deep in the negative tail'
    off = MR.param_offsets()
    flat = C.params(0.1, padding=2.0 ** -7)
    P = MR.param_views(torch.tensor(flat))
    for name, cols in MR.PADDING.items():
        assert (P[name][:, list(cols)] == 2.0 ** -7).all() and float(P[name].abs().max()) > 2.0 ** -7
    assert off[22] == flat.size


def _oracle_params(P):
    d = {}
    for l in range(7):
        d[f'mlp_feat.{l}.weight'], d[f'mlp_feat.{l}.bias'] = P[f'W{l}'][:, :{0: 63, 4: 319}.get(l, 256)], P[f'b{l}']
    d['mlp_feat.7.weight'], d['mlp_feat.7.bias'] = torch.cat([P['wd'][None], P['W7']], 0), torch.cat([P['bd'], P['b7']])
    d['mlp_rgb.0.weight'], d['mlp_rgb.0.bias'] = P['R0'][:, :283], P['br0']
    d['mlp_rgb.1.weight'], d['mlp_rgb.1.bias'] = P['R1'], P['br1']
    return {k: v.detach().clone().to(F64).requires_grad_(True) for k, v in d.items()}


@pytest.mark.parametrize('progress', ['partly', 'open'])
def test_chained_float64_stages_are_the_oracle_and_its_autograd(progress):
    R, S = 7, 9
    M = R * S
    c = C.case(R, S, progress, bd=0.1)
    P = {k: v.to(F64) for k, v in MR.param_views(torch.tensor(c['flat'])).items()}
    center, ray, depth, g_rgb, g_den = (torch.tensor(c[k]).to(F64) for k in ('center', 'ray', 'depth', 'g_rgb', 'g_den'))
    p = C.PROGRESS[progress]
    bands = torch.cat([SN.band_weights(p, C.BARF_C2F, L, F64) for L in (SN.L_3D, SN.L_VIEW)])
    # the chain
    pts = center[:, None] + ray[:, None] * depth[..., None]
    unit = ray / ray.norm(dim=-1, keepdim=True)
    enc = torch.zeros(M, 64, dtype=F64)
    enc[:, :63] = SN.encode(pts, SN.L_3D, bands[:10]).reshape(M, 63)
    view = torch.zeros(M, 32, dtype=F64)
    view[:, :27] = SN.encode(unit, SN.L_VIEW, bands[10:]).repeat_interleave(S, 0)
    a, x = [], enc
    for l in range(8):
        y = MR.layer(x, P[f'W{l}'], P[f'b{l}'])[0]
        x = torch.cat([y, enc], 1) if l == 3 else torch.cat([y, view], 1) if l == 7 else y
        a.append(x)
    raw = MR.raw_density(a[6], P['wd'], P['bd'])[0]
    dens = MR.density(raw)[0]
    h = MR.layer(a[7], P['R0'], P['br0'])[0]
    rgb = MR.rgb(h, P['R1'], P['br1'])[0]
    G = {}
    dH = MR.d_hidden(g_rgb, rgb, P['R1'], h)[0]
    G['R1'], G['br1'] = MR.grad_R1(g_rgb, rgb, h)[0], MR.grad_br1(g_rgb, rgb)[0]
    G['R0'], G['br0'] = MR.grad_w(dH, a[7])[0], MR.grad_b(dH)[0]
    dHsum = MR.ray_sum(dH, R, S)[0]
    dView = MR.d_view(dHsum, P['R0'])[0]
    draw = MR.d_raw(g_den, raw)[0]
    G['wd'], G['bd'] = MR.grad_wd(draw, a[6])[0], MR.grad_bd(draw)[0]
    d7 = MR.data_grad(dH, P['R0'][:, :256], a[7][:, :256])[0]
    G['W7'], G['b7'] = MR.grad_w(d7, a[6])[0], MR.grad_b(d7)[0]
    DY = {6: MR.data_grad(torch.cat([d7, draw[:, None]], 1), torch.cat([P['W7'], P['wd'][None]], 0), a[6])[0]}
    for l in range(6, 0, -1):
        DY[l - 1] = MR.data_grad(DY[l], P[f'W{l}'][:, :256], a[l - 1][:, :256])[0]
    for l in range(7):
        G[f'W{l}'], G[f'b{l}'] = MR.grad_w(DY[l], enc if l == 0 else a[l - 1])[0], MR.grad_b(DY[l])[0]
    dEncS, dEnc0 = MR.d_enc(DY[4], P['W4'][:, 256:320])[0], MR.d_enc(DY[0], P['W0'])[0]
    (gc, _, _), (gr, _, _) = MR.ray_grads(center, ray, depth, bands, dEnc0, dEncS, dView)
    # the oracle on the same linear piece
    OP = _oracle_params(P)
    co, ro = center.clone().requires_grad_(True), ray.clone().requires_grad_(True)
    masks = [t[:, :256] > 0 for t in a] + [h > 0]
    rgb_o, dens_o = SN.mlp(OP, co[:, None] + ro[:, None] * depth[..., None], ro, p, C.BARF_C2F, masks=masks)
    ((rgb_o.reshape(M, 3) * g_rgb).sum() + (dens_o.reshape(M) * g_den).sum()).backward()

    def same(name, got, ref):
        got, ref = got.detach(), ref.detach()
        assert got.shape == ref.shape, name
        assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-300), name

    same('rgb', rgb, rgb_o.reshape(M, 3))
    same('density', dens, dens_o.reshape(M))
    same('g_center', gc, co.grad)
    same('g_ray', gr, ro.grad)
    for l in range(7):
        used = {0: 63, 4: 319}.get(l, 256)
        same(f'g.W{l}', G[f'W{l}'][:, :used], OP[f'mlp_feat.{l}.weight'].grad)
        assert (G[f'W{l}'][:, used:] == 0).all()
        same(f'g.b{l}', G[f'b{l}'], OP[f'mlp_feat.{l}.bias'].grad)
    same('g.W7', torch.cat([G['wd'][None], G['W7']], 0), OP['mlp_feat.7.weight'].grad)
    same('g.b7', torch.cat([G['bd'], G['b7']]), OP['mlp_feat.7.bias'].grad)
    same('g.R0', G['R0'][:, :283], OP['mlp_rgb.0.weight'].grad)
    assert (G['R0'][:, 283:] == 0).all()
    same('g.br0', G['br0'], OP['mlp_rgb.0.bias'].grad)
    same('g.R1', G['R1'], OP['mlp_rgb.1.weight'].grad)
    same('g.br1', G['br1'], OP['mlp_rgb.1.bias'].grad)


MARGIN_CASES = [((7, 9), 'open', 0.1, 'random'), ((29, 67), 'partly', 20.0, 'random'), ((5, 13), 'closed', -30.0, 'random'),
                ((5, 51), 'open', 20.0, 'density_only'), ((5, 13), 'open', 0.1, 'zero')]


def test_float32_in_a_third_association_passes_the_rule_and_prints_its_margin():
    need = {}
    for (R, S), progress, bd, upstream in MARGIN_CASES:
        run = MR.emulate32(C.case(R, S, progress, bd, upstream))
        for name, got, (r64, r32, scale) in MR.all_stages(run):
            assert bool(torch.isfinite(got).all()), name
            check(f'{R}x{S} {progress} bd={bd} {upstream}: {name}', got, r64, r32, scale)
            need[name] = max(need.get(name, 0.0), float(MR.ulps_needed(got, r64, r32, scale)))
        for what, ok in MR.exact_promises(run):
            assert ok, what
        if upstream != 'random':
            zero = [k for k in MR.PARAM_NAMES if upstream == 'zero' or k in ('R0', 'br0', 'R1', 'br1')]
            assert all(bool((run.G[k] == 0).all()) for k in zero), 'no upstream gradient: exactly zero'
            assert bool((run.X['dH'] == 0).all()) and bool((run.X['dView'] == 0).all())
        if upstream == 'zero':
            assert bool((run.g_center == 0).all()) and bool((run.g_ray == 0).all())
    print('ulps needed by float32 numpy in a third association (8 allowed):')
    print('  ' + '  '.join(f'{k} {v:.2f}' for k, v in need.items()))
    assert max(need.values()) <= 8
