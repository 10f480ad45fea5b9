"""CPU checks of what tests/test_hip_object_mlp_kernels.py rests on (tests/object_mlp_reference.py, tests/object_mlp_cases.py):
  * the restated layouts are those of the library: workspace sizes, parameter counts, and the views round-trip on a synthetic block;
  * the float64 stage references, chained, ARE oracle.voxurf_oracle.warp_mlp (values; its Jacobian and every gradient through a double
    backward) and tests/analytic_model.warp_forward / warp_backward, and oracle.voxurf_oracle.rgbnet_mlp with autograd, to 1e-12 -
    on inputs none of whose float64 pre-activations lies within 1e-6 of zero (asserted, not filtered for);
  * a float32 numpy pass in a third association (object_mlp_reference.emulate32_*) passes helpers.check at the default 8 ulps on
    every stage, case and image of the blocks, with every row on its OWN scale; the ulps it needs are printed - the CPU column of
    the table in DESIGN.md, section 5;
  * the planted cases have the properties the GPU tests rest on."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import voxurf_oracle as O
from tests import analytic_model as AM
from tests import object_mlp_cases as C
from tests import object_mlp_reference as MR
from tests.helpers import check

F64 = torch.float64


def test_layouts_are_the_library_s():
    from poseprobe_amd import ops
    assert (MR.WARP_PARAMS, MR.RGB_PARAMS) == (ops.WARP_PARAMS, ops.RGBNET_PARAMS)
    for cap in (1, 7, 567, 2245, 54613):
        assert MR.workspace_floats(cap) == ops.mlp_workspaces(cap), cap


def test_layout_views_round_trip_on_a_synthetic_block():
    cap = 5
    na, ns = MR.workspace_floats(cap)['warp']
    acts, scr = torch.arange(na, dtype=torch.float32), torch.arange(ns, dtype=torch.float32)
    X, S = MR.warp_acts_view(acts, cap), MR.warp_scratch_view(scr, cap)
    for l, s, r, n in ((0, 0, 0, 0), (3, 4, 3, 127), (2, 1, 2, 64)):
        assert float(X[l, 4 * s + r, n]) == l * cap * 4 * 128 + (4 * s + r) * 128 + n
    assert float(S[2, 4 * 4 + 3, 127]) == 3 * cap * 4 * 128 - 1 and ns - 3 * cap * 4 * 128 == MR.TAIL
    na, ns = MR.workspace_floats(cap)['rgbnet']
    H, S = MR.rgb_acts_view(torch.arange(na, dtype=torch.float32), cap), MR.rgb_scratch_view(torch.arange(ns, dtype=torch.float32), cap)
    assert float(H[2, 4, 127]) == na - 1 and float(S[1, 2, 3]) == cap * 128 + 2 * 128 + 3
    flat = torch.arange(MR.WARP_PARAMS, dtype=torch.float32)
    P = MR.warp_param_views(flat)
    assert float(P['W0'][127, 2]) == 383 and float(P['b0'][0]) == 384 and float(P['W1'][0, 0]) == 512
    assert float(P['W4'][3, 127]) == MR.WARP_PARAMS - 5 and float(P['b4'][3]) == MR.WARP_PARAMS - 1
    assert [int(P[f'W{l}'][0, 0]) for l in range(5)] == [0, 512, 512 + 16512, 512 + 2 * 16512, 512 + 3 * 16512]
    R = MR.rgb_param_views(torch.arange(MR.RGB_PARAMS, dtype=torch.float32))
    assert [int(R[f'W{l}'][0, 0]) for l in range(4)] == [0, 8320, 8320 + 16512, 8320 + 2 * 16512] and float(R['b3'][2]) == MR.RGB_PARAMS - 1
    # the packing of the cases is the engine's
    from poseprobe_amd.engine import pack_rgbnet, pack_warp
    from tests.test_hip_mlp import _rgb_params, _warp_params
    assert np.array_equal(C.warp_case(3)['flat'][:MR.WARP_PARAMS], pack_warp(_warp_params(3)).numpy())
    assert np.array_equal(C.rgb_case(3)['flat'][:MR.RGB_PARAMS], pack_rgbnet(_rgb_params(5)).numpy())


def _same(name, got, ref):
    got, ref = got.detach(), ref.detach()
    assert got.shape == ref.shape, name
    assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-300), name


def _assert_no_pre_activation_near_zero(pre):
    """No float64 pre-activation within 1e-6 of zero, so that no ReLU state depends on the evaluation order.  With the weights scaled
    by 1e-3 a layer's pre-activations are themselves 1e-3 .. 1e-9: there the distance is taken relative to the layer's largest."""
    for l, p in enumerate(pre):
        assert float(p.abs().min()) > 1e-6 * min(1.0, float(p.abs().max())), f'layer {l}: a pre-activation within 1e-6 of zero: choose another seed'


def _open(rows):
    return torch.ones(rows, 128, dtype=F64)


@pytest.mark.parametrize('scales', C.SCALES)
def test_chained_float64_warp_stages_are_the_oracle_and_the_analytic_model(scales):
    M = 17
    c = C.warp_case(M, scales=scales)
    P = {k: v.to(F64) for k, v in MR.warp_param_views(torch.tensor(c['flat'])).items()}
    pts, og, rng = torch.tensor(c['pts']).to(F64), torch.tensor(c['out_grad']).to(F64), float(c['out_range'])
    # the chain: every stage on the previous stage's float64 value, its gates from its own primal rows
    pre = [pts @ P['W0'].T + P['b0']]
    stored0 = torch.zeros(4 * M, 128, dtype=F64)
    stored0[::4] = torch.relu(pre[0])
    X = [MR.warp_x0(pts, P['W0'], P['b0'], stored0)[0]]
    for l in (1, 2, 3):
        pre.append((X[-1] @ P[f'W{l}'].T)[::4] + P[f'b{l}'])
        first = MR.hidden(X[-1], P[f'W{l}'], P[f'b{l}'], _open(4 * M), 4)[0]
        X.append(MR.hidden(X[-1], P[f'W{l}'], P[f'b{l}'], first, 4)[0])
    _assert_no_pre_activation_near_zero(pre)
    out = MR.warp_out(X[3], P['W4'], P['b4'], rng)[0]
    g = (og * rng).reshape(4 * M, 4)
    Y = {3: MR.data_grad(g, P['W4'], X[3], 4)[0]}
    for l in (2, 1, 0):
        Y[l] = MR.data_grad(Y[l + 1], P[f'W{l + 1}'], X[l], 4)[0]
    G = {'W4': MR.grad_w(g, X[3])[0], 'b4': MR.grad_b(g, 4)[0]}
    for l in (3, 2, 1):
        G[f'W{l}'], G[f'b{l}'] = MR.grad_w(Y[l], X[l - 1])[0], MR.grad_b(Y[l], 4)[0]
    G['W0'] = torch.einsum('sn,si->ni', Y[0][::4], pts) + Y[0].view(M, 4, 128)[:, 1:].sum(0).T
    G['b0'] = Y[0][::4].sum(0)
    pts_grad = Y[0][::4] @ P['W0']
    # the oracle: values, the Jacobian by autograd.grad(create_graph=True) as the reference forms it, gradients by a double backward
    OP = {'warp': [(P[f'W{l}'].clone().requires_grad_(True), P[f'b{l}'].clone().requires_grad_(True)) for l in range(5)]}
    p = pts.clone().requires_grad_(True)
    o3, o1 = O.warp_mlp(OP, SimpleNamespace(output_range=rng), p)
    o = torch.cat([o3, o1], 1)                                                        # [M, 4]
    J = torch.stack([torch.autograd.grad(o[:, j].sum(), p, create_graph=True)[0] for j in range(4)], 2)      # [M, i, j]
    full = torch.cat([o[:, None], J], 1)                                              # [M, 4 rows, 4]
    _same('out', out.view(M, 4, 4), full)
    (full * og.view(M, 4, 4)).sum().backward()
    _same('pts_grad', pts_grad, p.grad)
    for l in range(5):
        _same(f'W{l}bar', G[f'W{l}'], OP['warp'][l][0].grad)
        _same(f'b{l}bar', G[f'b{l}'], OP['warp'][l][1].grad)
    # the analytic model (float64 through the default dtype: it builds its own zeros)
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    try:
        warp = [(P[f'W{l}'], P[f'b{l}']) for l in range(5)]
        a_out, a_acts = AM.warp_forward(warp, pts, rng)
        a_grads, a_pbar = AM.warp_backward(warp, a_acts, og.view(M, 4, 4), rng)
    finally:
        torch.set_default_dtype(old)
    _same('analytic out', out.view(M, 4, 4), a_out)
    for l in range(4):
        _same(f'analytic X{l}', X[l].view(M, 4, 128), a_acts[l + 1])
    _same('analytic pts_grad', pts_grad, a_pbar)
    for l in range(5):
        _same(f'analytic W{l}bar', G[f'W{l}'], a_grads[l][0])
        _same(f'analytic b{l}bar', G[f'b{l}'], a_grads[l][1])


@pytest.mark.parametrize('scales', C.SCALES)
def test_chained_float64_rgbnet_stages_are_the_oracle_and_its_autograd(scales):
    M = 33
    c = C.rgb_case(M, scales=scales)
    P = {k: v.to(F64) for k, v in MR.rgb_param_views(torch.tensor(c['flat'])).items()}
    feat, gr = torch.tensor(c['feat']).to(F64), torch.tensor(c['rgb_grad']).to(F64)
    H, x, pre = [], feat, []
    for l in range(3):
        pre.append(x @ P[f'W{l}'].T + P[f'b{l}'])
        H.append(MR.hidden(x, P[f'W{l}'], P[f'b{l}'], _open(M), 1)[0])
        x = H[-1]
    _assert_no_pre_activation_near_zero(pre)
    rgb = MR.rgb_out(H[2], P['W3'], P['b3'])[0]
    gl = MR._gl(gr, rgb)
    Y = {2: (gl @ P['W3']) * (H[2] > 0)}
    Y[1] = MR.data_grad(Y[2], P['W2'], H[1], 1)[0]
    Y[0] = MR.data_grad(Y[1], P['W1'], H[0], 1)[0]
    G = {'W3': gl.T @ H[2], 'b3': gl.sum(0)}
    for l in (2, 1, 0):
        G[f'W{l}'], G[f'b{l}'] = MR.grad_w(Y[l], feat if l == 0 else H[l - 1])[0], MR.grad_b(Y[l], 1)[0]
    feat_grad = Y[0] @ P['W0']
    OP = {'rgbnet': [(P[f'W{l}'][:, :MR.RGB_IN if l == 0 else None].clone().requires_grad_(True), P[f'b{l}'].clone().requires_grad_(True))
                     for l in range(4)]}
    f = feat[:, :MR.RGB_IN].clone().requires_grad_(True)
    rgb_o = torch.sigmoid(O.rgbnet_mlp(OP, f))
    (rgb_o * gr).sum().backward()
    _same('rgb', rgb, rgb_o)
    _same('feat_grad', feat_grad[:, :MR.RGB_IN], f.grad)
    assert bool((feat_grad[:, MR.RGB_IN:] == 0).all())
    for l in range(4):
        _same(f'W{l}bar', G[f'W{l}'][:, :MR.RGB_IN] if l == 0 else G[f'W{l}'], OP['rgbnet'][l][0].grad)
        _same(f'b{l}bar', G[f'b{l}'], OP['rgbnet'][l][1].grad)
    assert bool((G['W0'][:, MR.RGB_IN:] == 0).all())


WARP_MARGIN = [(17, 20, None, 'full'), (55, 55, None, 'lean'), (55, 55, None, 'layered'), (567, 567, None, 'lean'), (55, 58, 'some_upstream', 'lean'),
               (55, 55, 'no_upstream', 'full'), (55, 55, 'dead_silent', 'lean'), (55, 55, 'zero_gate', 'full'), (55, 55, 'zero_gate', 'lean'),
               (55, 55, 'range', 'lean'), (55, 55, 'range', 'full')]
RGB_MARGIN = [(33, 35, None, 'full'), (197, 197, None, 'layered'), (2245, 2245, None, 'full'), (197, 197, 'some_upstream', 'full'),
              (197, 197, 'no_upstream', 'full'), (197, 197, 'dead_silent', 'full'), (197, 197, 'range', 'full')]


def _margin(net, cases, emulate, stages, promises, make):
    need = {}
    for i, (M, cap, plant, form) in enumerate(cases):
        for scales in C.SCALES:
            run = emulate(make(M, cap=cap, scales=scales, plant=plant), form)
            tag = f'{net} M = {M} capacity {cap} {plant} {form} scales {scales}'
            for name, got, (r64, r32, scale) in stages(run):
                assert bool(torch.isfinite(got).all()), f'{tag}: {name}'
                check(f'{tag}: {name}', got, r64, r32, scale)
                key = f'{name}[range]' if plant == 'range' else name
                need[key] = max(need.get(key, 0.0), float(MR.ulps_needed(got, r64, r32, scale)))
            for what, ok in promises(run):
                assert ok, f'{tag}: {what}'
            if net == 'warp' and form != 'lean':
                got, want = MR.x0_tangent_rows(run)
                assert torch.equal(MR.bits(got), MR.bits(want)), f'{tag}: the tangent rows of X0'
            if plant == 'no_upstream':
                assert all(bool((v == 0).all()) for v in run.G.values()), f'{tag}: no upstream gradient, exactly zero gradients'
    print(f'{net}: ulps needed by float32 numpy in a third association (8 allowed), every row on its own scale:')
    print('  ' + '  '.join(f'{k} {v:.2f}' for k, v in need.items()))
    assert max(need.values()) <= 8


def test_float32_in_a_third_association_passes_the_rule_and_prints_its_margin_warp():
    _margin('warp', WARP_MARGIN, MR.emulate32_warp, MR.warp_stages, MR.warp_exact_promises, C.warp_case)


def test_float32_in_a_third_association_passes_the_rule_and_prints_its_margin_rgbnet():
    _margin('rgbnet', RGB_MARGIN, MR.emulate32_rgb, MR.rgb_stages, MR.rgb_exact_promises, C.rgb_case)


def test_planted_cases_have_their_properties():
    c = C.warp_case(55, plant='zero_gate')
    P = MR.warp_param_views(torch.tensor(c['flat']))
    assert (c['pts'][C.ZERO_SAMPLE] == 0).all() and all(float(P['b0'][n]) == 0 and bool((P['W0'][n] != 0).all()) for n in C.ZERO_UNITS)
    run = MR.emulate32_warp(c, 'full')
    x0 = run.X[0][4 * C.ZERO_SAMPLE:4 * C.ZERO_SAMPLE + 4][:, list(C.ZERO_UNITS)]
    assert bool((MR.bits(x0) == 0).all()), 'the contract: a primal pre-activation of +0 closes the gate, the tangent rows are +0'
    for net, make, emulate, hid, acts in (('warp', C.warp_case, MR.emulate32_warp, 2, 'X'), ('rgbnet', C.rgb_case, MR.emulate32_rgb, 1, 'H')):
        M = 55 if net == 'warp' else 197
        run = emulate(make(M, plant='dead_silent'), 'full')
        A = getattr(run, acts)[hid]
        assert bool((MR.bits(A[:, list(C.DEAD) + list(C.SILENT)][:M * (4 if net == 'warp' else 1)]) == 0).all()), f'{net}: dead and silent units are +0'
        assert float(A[:, [0, 1, 2]].abs().nan_to_num().max()) > 0
        c = make(M, plant='some_upstream')
        g = c['out_grad' if net == 'warp' else 'rgb_grad']
        assert (g[::3] == 0).all() and (g[1::3] != 0).any()
        c, plain = make(M, plant='range'), make(M)
        k, s = ('pts', C.RANGE_SAMPLE['warp']) if net == 'warp' else ('feat', C.RANGE_SAMPLE['rgbnet'])
        assert np.array_equal(c[k][s], plain[k][s] * C.RANGE_FACTOR) and np.array_equal(np.delete(c[k], s, 0), np.delete(plain[k], s, 0))
        assert MR.HALF_ROWS <= s * (4 if net == 'warp' else 1) < 2 * MR.HALF_ROWS
    assert C.second_tile_sizes(256) == (16 * 256 + 23, 64 * 256 + 69)
