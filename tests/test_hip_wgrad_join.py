"""The join scope of the weight gradients (pp_wgrad_join_begin / pp_wgrad_join_end): inside it pp_rgbnet_bwd leaves its
weight-gradient chain as a record in the context and the next warp chain carries the three products in its own launch
(k_wgrad_join_s: six layers, one grid).

Operands and float64 references are those of tests/test_hip_wgrad_split.py.  The warp net rides in lean form only, so its operands
are given as the lean image (16 output gradients per sample, primal rows of X0) AND as the full form that image stands for; the
fp32 chain and the float64 reference work on the full form.  rgbnet's record is made by pp_rgbnet_bwd itself, whose data-gradient
kernel writes Ybar: Y of the reference is read back from the buffer it leaves, X is what was prepared.
"""
import pytest
import torch

from tests.test_hip_wgrad_split import DEV, WARP_BASE, _assert_as_accurate, _errors, _layout, _operands

pytestmark = pytest.mark.gpu

W4_OFF = WARP_BASE + 3 * (128 * 128 + 128)                      # W0 b0 | W1 b1 | W2 b2 | W3 b3 | W4 b4
RGB_W3 = 128 * 64 + 128 + 2 * (128 * 128 + 128)                 # rgbnet: W0 b0 | W1 b1 | W2 b2 | W3 b3
NAN = float('nan')


def shares():
    """Work-groups per warp layer / 128-wide rgbnet layer / input layer before the clamp to the tile counts (poseprobe_hip.h):
    10 : 10 : 10 : 4 : 4 : 3 of two work-groups per CU, rounded to nearest, the input layer taking the rest."""
    wgs = 2 * torch.cuda.get_device_properties(DEV).multi_processor_count
    nw, nd = (wgs * 10 + 20) // 41, (wgs * 4 + 20) // 41
    return nw, nd, max(wgs - 3 * nw - 2 * nd, 1)


def make_case(M, cap, seed):
    """Everything one joined launch at M samples reads.  Warp net: Y[0] = gate(X3) * (g W4) and the tangent rows of X[2] = X0 are
    what the lean form rebuilds; W4's entries are signed powers of two and g has 8 significant bits, so the rebuilt sums are exact
    in float32 whatever the order (up to cancellation beyond 24 bits, which changes nothing measurable)."""
    from poseprobe_amd import ops
    g = torch.Generator().manual_seed(seed)
    c = dict(M=M, cap=cap, count=torch.tensor([M], dtype=torch.int32, device=DEV))
    # ---- warp net
    rc, na, ns, npg, _ = _layout('warp', cap)
    rows = 4 * M
    Y, X, _, _, _ = _operands('warp', M, cap, g)
    X3 = torch.randn(rows, 128, generator=g)
    g16 = torch.randn(rows, 4, generator=g).bfloat16().float()
    W4 = torch.exp2(torch.randint(-2, 3, (4, 128), generator=g).float()) * (torch.randint(0, 2, (4, 128), generator=g).float() * 2 - 1)
    W0 = torch.randn(128, 3, generator=g)
    prim = torch.arange(rows) // 4 * 4                                       # the primal row of each row's sample
    Y[0] = torch.where(X3[prim] > 0, g16.double() @ W4.double(), torch.zeros((), dtype=torch.float64)).float()
    tang = (torch.arange(rows) % 4 != 0)
    X0 = X[2].clone()
    for i in range(3):
        X0[i + 1::4] = torch.where(X0[0::4] > 0, W0[:, i][None, :].expand(M, 128), torch.zeros(()))
    X[2] = X0
    full_acts, full_scratch = torch.zeros(na), torch.zeros(ns)
    for i, slot in enumerate((2, 1, 0)):
        full_acts[slot * rc * 128:slot * rc * 128 + rows * 128] = X[i].reshape(-1)
        full_scratch[i * rc * 128:i * rc * 128 + rows * 128] = Y[i].reshape(-1)
    full_acts[3 * rc * 128:3 * rc * 128 + rows * 128] = X3.reshape(-1)
    lean_acts, lean_scratch = full_acts.clone(), full_scratch.clone()
    slot0 = lean_acts[:rows * 128].view(rows, 128)
    slot0[tang] = NAN                                                        # never read: the kernel rebuilds them
    lean_scratch[:rc * 128] = NAN
    lean_scratch[:rows * 4] = g16.reshape(-1)
    params = torch.zeros(ops.WARP_PARAMS)
    params[:384] = W0.reshape(-1)
    params[W4_OFF:W4_OFF + 512] = W4.reshape(-1)
    c['warp'] = dict(Y=Y, X=X, full_acts=full_acts.to(DEV), full_scratch=full_scratch.to(DEV), acts=lean_acts.to(DEV),
                     scratch=lean_scratch.to(DEV), params=params.to(DEV), npg=npg)
    # ---- rgbnet: X prepared, Y left by the data-gradient kernel
    rc, na, ns, npg, _ = _layout('rgbnet', cap)
    _, Xr, acts, _, feat = _operands('rgbnet', M, cap, g)
    acts[2 * rc * 128:2 * rc * 128 + M * 128] = torch.relu(torch.randn(M * 128, generator=g)).to(DEV)      # X2 gates Ybar2
    c['rgb'] = dict(X=Xr, acts=acts, feat=feat, scratch=torch.zeros(ns, device=DEV), npg=npg,
                    params=(torch.randn(ops.RGBNET_PARAMS, generator=g) * 0.1).to(DEV),
                    rgb=torch.sigmoid(torch.randn(cap, 3, generator=g)).to(DEV), rgb_grad=torch.randn(cap, 3, generator=g).to(DEV),
                    feat_grad=torch.zeros(cap, 64, device=DEV))
    return c


def rgbnet_bwd(c, grad, ctx):
    from poseprobe_amd import ops
    r = c['rgb']
    ops.rgbnet_bwd(r['params'], r['feat'], r['acts'], r['rgb'], r['rgb_grad'], c['count'], c['cap'], r['scratch'], grad, r['feat_grad'], ctx)


def warp_weights(c, grad, ctx, count=None):
    from poseprobe_amd import ops
    w = c['warp']
    ops.warp_bwd_weights(w['acts'], w['scratch'], c['count'] if count is None else count, c['cap'], grad, 1, ctx)


def joined(c, grad_w, grad_r):
    """the joined launch: lean scope, join scope, the deferring call, the warp chain that carries the record"""
    from poseprobe_amd import ops
    ctx = ops.Context()
    w = c['warp']
    ops.warp_lean_begin(w['acts'], w['scratch'], w['params'], ctx)
    ops.wgrad_join_begin(ctx)
    rgbnet_bwd(c, grad_r, ctx)
    warp_weights(c, grad_w, ctx)
    ops.wgrad_join_end(ctx, launch_pending=False)               # nothing is pending any more: dropping must lose nothing
    ops.warp_lean_end(ctx)
    torch.cuda.synchronize()


def rgb_Y(c):
    r, M, cap = c['rgb'], c['M'], c['cap']
    return [r['scratch'][i * cap * 128:i * cap * 128 + M * 128].view(M, 128).cpu() for i in range(3)]


def hidden(net, cap):
    """bool mask over params_grad: the three layers' Wbar and bbar"""
    _, _, _, npg, layers = _layout(net, cap)
    m = torch.zeros(npg, dtype=torch.bool, device=DEV)
    for off, kx in layers:
        m[off:off + 128 * kx + 128] = True
    return m


def errors_of(net, grad, Y, X, cap, M, what):
    """as tests/test_hip_wgrad_split.py::_errors does for one result: relative rms error of the three Wbar against float64, bias sums
    and padded input columns checked"""
    _, _, _, _, layers = _layout(net, cap)
    e = []
    for i, (off, kx) in enumerate(layers):
        ref = Y[i].to(DEV).double().T @ X[i].to(DEV).double()
        got = grad[off:off + 128 * kx].view(128, kx).double()
        refb = Y[i][::4 if net == 'warp' else 1].to(DEV).double().sum(0)
        gb = grad[off + 128 * kx:off + 128 * kx + 128].double()
        assert float((gb - refb).abs().max()) <= 1e-5 * float(refb.abs().max()) + 1e-30, f'{net} bias {i} ({what})'
        if net == 'rgbnet' and kx == 64:
            assert bool((got[:, 57:] == 0).all()), f'padded input columns ({what})'
        den = float((ref ** 2).mean().sqrt())
        if den == 0.0:
            assert bool((got == 0).all()), f'{net} layer {i} ({what}): nonzero gradient of no rows'
            e.append(0.0)
        else:
            e.append(float(((got - ref) ** 2).mean().sqrt()) / den)
    return e


def full_grid_M():
    """smallest M at which the half-grid rule is off: 4 M rows (16 samples per tile) in at least 8 tiles per work-group of a warp layer"""
    return 16 * (8 * shares()[0] - 1) + 1


@pytest.mark.parametrize('M', [0, 1, 17, 65, 4133, 'full', 54600])
def test_joined_launch_against_float64(M):
    """Both nets at once.  0: every work-group empty; 1: one rgbnet row, four warp rows; 17: a partial 16-row piece; 65: a ragged
    second rgbnet tile; 4133: several rounds on half the grid, the last round shared in 16-row pieces; 'full': the smallest M at
    which every work-group works (8 tiles per warp work-group; 15 985 at 256 CUs); 54 600: the benchmark's size.
    Bound: that of the separate launches - the split chain's relative rms error at most 1.25 x the fp32 chain's on the same
    operands, 1.5 x where the warp net has more than 100 k rows, with the floor of _assert_as_accurate.  At 54 600 samples a
    work-group of the joined launch sums about 1750 warp rows (separate launch: 1285) and 1090 / 1480 rgbnet rows (590 / 780).
    Measured on an MI355X (256 CUs) at 54 600, joined / fp32 chain per layer: warp 1.27, 1.47, 1.19, rgbnet 1.36, 1.47, 1.26; two
    runs differ by about 1 %.  (Shares by rows alone, 16 : 16 : 16 : 4 : 4 : 3, gave rgbnet 1.60, 1.63, 1.69: not shipped.)"""
    if M == 'full':
        M = full_grid_M()
        nw, nd, nf = shares()
        assert (4 * M + 63) // 64 == 8 * nw == (4 * (M - 1) + 63) // 64 + 1
    cap = max(M, 40) if M == 0 else M
    c = make_case(M, cap, 2000 + M)
    w, r = c['warp'], c['rgb']
    grad_w, grad_r = torch.zeros(w['npg'], device=DEV), torch.zeros(r['npg'], device=DEV)
    joined(c, grad_w, grad_r)
    ratio = 1.5 if 4 * M > 100000 else 1.25
    Yr = rgb_Y(c)
    for net, grad, Y, X, sep in (('warp', grad_w, w['Y'], w['X'], (w['full_acts'], w['full_scratch'], None)),
                                 ('rgbnet', grad_r, Yr, r['X'], (r['acts'], r['scratch'], r['feat']))):
        what = f'joined launch, M = {M}'
        e_join = errors_of(net, grad, Y, X, cap, M, what)
        e_sep = _errors(net, M, cap, Y, X, *sep)                # fp32 chain [0] and split chain [16] in launches of their own
        print(f'{net} M = {M}: fp32 chain {e_sep[0]}, separate split chain {e_sep[16]}, joined {e_join}, ratios '
              f'{[b / a if a else 0.0 for a, b in zip(e_sep[0], e_join)]}')
        _assert_as_accurate(net, {0: e_sep[0], 16: e_join}, what, ratio)


def single(c):
    """M = 1, capacity 1: one work-group per layer on every route, so every sum has one order"""
    assert c['M'] == 1 and c['cap'] == 1


def rgb_reference(c):
    """what pp_rgbnet_bwd leaves outside any scope: the data-gradient kernel's entries and the chain's"""
    from poseprobe_amd import ops
    grad = torch.zeros(c['rgb']['npg'], device=DEV)
    rgbnet_bwd(c, grad, ops.Context())
    torch.cuda.synchronize()
    return grad


def test_who_launches_the_recorded_chain(monkeypatch):
    """Calls through a recorder around _lib.call; results compared.  At (1, 1) every route adds the same terms in the same order."""
    from poseprobe_amd import _lib, ops
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    c = make_case(1, 1, 7)
    single(c)
    w, r = c['warp'], c['rgb']
    want_r = rgb_reference(c)
    hid = hidden('rgbnet', 1)
    assert float(want_r[hid].abs().max()) > 0
    want_w = torch.zeros(w['npg'], device=DEV)
    ctx = ops.Context()
    ops.warp_lean_begin(w['acts'], w['scratch'], w['params'], ctx)
    warp_weights(c, want_w, ctx)
    # (rgbnet's scratch and feat_grad are the data-gradient kernel's to write)
    before = {(net, k): c[net][k].clone() for net, keys in (('warp', ('acts', 'scratch', 'params')),
                                                            ('rgb', ('acts', 'feat', 'params', 'rgb', 'rgb_grad'))) for k in keys}

    def fresh():
        return torch.zeros(w['npg'], device=DEV), torch.zeros(r['npg'], device=DEV)

    # the record rides: nothing of the chain before the warp call, everything after it
    gw, gr = fresh()
    ops.wgrad_join_begin(ctx)
    rgbnet_bwd(c, gr, ctx)
    torch.cuda.synchronize()
    assert float(gr[hid].abs().max()) == 0 and torch.equal(gr[~hid], want_r[~hid]), 'the chain was not deferred'
    warp_weights(c, gw, ctx)
    torch.cuda.synchronize()
    assert torch.equal(gr, want_r) and torch.equal(gw, want_w), 'joined launch at one work-group per layer'
    ops.wgrad_join_end(ctx)

    # a foreign count tensor, then another stream, on the warp call: rgbnet's chain was launched on its own, the warp call is today's
    side = torch.cuda.Stream()
    for how in ('count', 'stream'):
        gw, gr = fresh()
        ops.wgrad_join_begin(ctx)
        rgbnet_bwd(c, gr, ctx)
        if how == 'count':
            warp_weights(c, gw, ctx, count=c['count'].clone())
        else:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                warp_weights(c, gw, ctx)
        torch.cuda.synchronize()
        assert torch.equal(gr, want_r) and torch.equal(gw, want_w), f'foreign {how}'
        ops.wgrad_join_end(ctx, launch_pending=False)
        torch.cuda.synchronize()
        assert torch.equal(gr, want_r), f'foreign {how}: something was still pending'

    # scope closed with nothing following: launched on its own = ops.rgbnet_bwd_weights on the same buffers
    _, gr = fresh()
    ops.wgrad_join_begin(ctx)
    rgbnet_bwd(c, gr, ctx)
    ops.wgrad_join_end(ctx)
    staged = torch.zeros_like(gr)
    ops.rgbnet_bwd_weights(r['feat'], r['acts'], r['scratch'], c['count'], 1, staged, 1, ctx)
    torch.cuda.synchronize()
    assert torch.equal(gr[hid], staged[hid]) and torch.equal(gr, want_r), 'chain launched by wgrad_join_end'

    # launch_pending = 0: dropped, params_grad untouched
    _, gr = fresh()
    gr[hid] = 7.0
    ops.wgrad_join_begin(ctx)
    rgbnet_bwd(c, gr, ctx)
    ops.wgrad_join_end(ctx, launch_pending=False)
    gw, _ = fresh()
    warp_weights(c, gw, ctx)                                    # and nothing is left for a later warp call
    torch.cuda.synchronize()
    assert bool((gr[hid] == 7.0).all()) and torch.equal(gr[~hid], want_r[~hid]) and torch.equal(gw, want_w), 'dropped record'

    # no scope: pp_rgbnet_bwd launches its chain; inside a scope pp_rgbnet_bwd_weights does, and another context is no part of it
    _, gr = fresh()
    rgbnet_bwd(c, gr, ctx)
    torch.cuda.synchronize()
    assert torch.equal(gr, want_r), 'outside a scope'
    ops.wgrad_join_begin(ctx)
    staged = torch.zeros_like(gr)
    ops.rgbnet_bwd_weights(r['feat'], r['acts'], r['scratch'], c['count'], 1, staged, 1, ctx)
    _, gr = fresh()
    rgbnet_bwd(c, gr, ops.Context())
    torch.cuda.synchronize()
    assert torch.equal(staged[hid], want_r[hid]) and torch.equal(gr, want_r), 'pp_rgbnet_bwd_weights / another context inside a scope'
    ops.wgrad_join_end(ctx, launch_pending=False)
    ops.warp_lean_end(ctx)
    assert names.count('pp_wgrad_join_begin') == names.count('pp_wgrad_join_end') == 6
    for (net, k), v in before.items():
        assert torch.equal(c[net][k].view(torch.int32), v.view(torch.int32)), f'{net} operand {k} was written'


@pytest.mark.parametrize('M,cap', [(1, 1), (65, 65)])
def test_joined_launch_stays_inside_both_gradient_blocks(M, cap):
    """The sentinel fence of tests/test_hip_wgrad_split.py around params_grad of BOTH nets: sentinels intact, only the hidden layers'
    entries written (rgbnet: also W3 / b3, the data-gradient kernel's), operands not written."""
    PAD, SENT = 16384, 0x7FC0DEAD
    c = make_case(M, cap, 5)
    w, r = c['warp'], c['rgb']
    ops_in = {('warp', k): w[k] for k in ('acts', 'scratch', 'params')}
    ops_in.update({('rgb', k): r[k] for k in ('acts', 'feat', 'params', 'rgb', 'rgb_grad')})
    before = {k: v.clone() for k, v in ops_in.items()}
    arenas, grads = {}, {}
    for net, npg in (('warp', w['npg']), ('rgbnet', r['npg'])):
        arenas[net] = torch.empty(npg + 2 * PAD, dtype=torch.int32, device=DEV).fill_(SENT).view(torch.float32)
        grads[net] = arenas[net][PAD:PAD + npg]
        grads[net].zero_()
    joined(c, grads['warp'], grads['rgbnet'])
    scratch_r = r['scratch'].clone()
    for net, npg in (('warp', w['npg']), ('rgbnet', r['npg'])):
        a = arenas[net].view(torch.int32)
        assert bool((a[:PAD] == SENT).all()), f'{net}: sentinels in front of the gradient block were overwritten'
        assert bool((a[PAD + npg:] == SENT).all()), f'{net}: sentinels behind the gradient block were overwritten'
        touched = hidden(net, cap)
        if net == 'rgbnet':
            touched[RGB_W3:RGB_W3 + 3 * 128 + 3] = True
        assert bool((grads[net][~touched] == 0).all()), f'{net}: entries outside the layers were written'
        assert float(grads[net][hidden(net, cap)].abs().max()) > 0
    for k, v in before.items():
        assert torch.equal(ops_in[k].view(torch.int32), v.view(torch.int32)), f'operand {k} was written'
    assert torch.equal(r['scratch'], scratch_r)


# ------------------------------------------------------------------------------------------------------------------ engine
JOIN = {'pp_wgrad_join_begin', 'pp_wgrad_join_end'}


def test_three_default_steps_against_the_two_launches(monkeypatch):
    """Two engines in lockstep from one state (tests/test_hip_step_launches.py), the default one and fuse_wgrad=False: everything in
    front of the float atomics bit for bit, what follows them within that file's bounds (which include flat.grad == 0 after the
    step).  Calls: the default engine opens and closes the scope once per step, the other one never."""
    from poseprobe_amd import _lib
    from tests.test_hip_side_by_side import small_engine
    from tests.test_hip_step_launches import adopt_state, compare_after_atomics, compare_exact
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    new, idx, jit = small_engine()
    old, _, _ = small_engine(fuse_wgrad=False)
    assert new.fuse_wgrad and new.side_by_side and not old.fuse_wgrad
    for e in (new, old):
        e.mlp_pack.zero_()
    for s in range(3):
        names.clear()
        new.train_step(idx, jit, 10 + s)
        assert all(names.count(n) == 1 for n in JOIN | {'pp_rgbnet_bwd', 'pp_warp_bwd'}), sorted(set(names))
        assert names.index('pp_wgrad_join_begin') < names.index('pp_rgbnet_bwd') < names.index('pp_warp_bwd') < names.index('pp_wgrad_join_end')
        names.clear()
        old.train_step(idx, jit, 10 + s)
        assert not (JOIN & set(names)) and names.count('pp_rgbnet_bwd') == 1
        torch.cuda.synchronize()
        compare_exact(new, old, f'step {s}')
        compare_after_atomics(new, old, f'step {s}')
        assert float(new.flat.grad.abs().max()) == 0.0 and float(old.flat.grad.abs().max()) == 0.0
        adopt_state(old, new)


def test_the_staged_warp_backward_picks_the_record_up(monkeypatch):
    """ops.warp_bwd replaced by its two stages, as bench.py --full does: pp_warp_bwd_weights carries the record; one step ends where
    the default engine's does, within the step bound."""
    from poseprobe_amd import _lib, ops
    from tests.test_hip_side_by_side import small_engine
    from tests.test_hip_step_launches import compare_after_atomics, compare_exact
    ref, idx, jit = small_engine()
    eng, _, _ = small_engine()
    for e in (ref, eng):
        e.mlp_pack.zero_()
    ref.train_step(idx, jit, 10)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])

    def staged_warp_bwd(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, ctx=None):
        stage2 = ops.warp_bwd_data(params, pts, acts, out_grad, count, capacity, out_range, scratch, params_grad, pts_grad, ctx)
        ops.warp_bwd_weights(acts, scratch, count, capacity, params_grad, stage2, ctx)
    monkeypatch.setattr(ops, 'warp_bwd', staged_warp_bwd)
    eng.train_step(idx, jit, 10)
    torch.cuda.synchronize()
    assert names.count('pp_warp_bwd_weights') == 1 and 'pp_warp_bwd' not in names and all(names.count(n) == 1 for n in JOIN)
    compare_exact(eng, ref, 'staged warp backward')
    compare_after_atomics(eng, ref, 'staged warp backward')


def test_the_deterministic_engine_keeps_the_two_launches(monkeypatch):
    """TrainEngine(deterministic=True) never opens the scope, and two runs stay equal bit for bit."""
    from poseprobe_amd import _lib
    from tests.test_hip_deterministic import assert_same_bits, run_small
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])
    a, b = run_small(3, deterministic=True), run_small(3, deterministic=True)
    assert not (JOIN & set(names)) and names.count('pp_rgbnet_bwd') == 6
    for s, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(x, y, f'step {s + 1}')
