"""The lean scope of the warp net (pp_warp_lean_begin / pp_warp_lean_end, option warp_lean): inside it the forward kernel leaves the
tangent rows of X0 unwritten, the data-gradient kernel writes the 16 scaled output gradients per sample instead of Ybar3, and the
weight-gradient kernel rebuilds both.  Everything the data path produces stays bit-identical to the full form, the hidden layers'
weight gradients agree with it to fp32 rounding, and a call outside the scope - another buffer, another context, after the end - is
the full form, untouched.

Exact comparisons are on the int32 view of the buffers (all of them start as a quiet-NaN sentinel no kernel produces), parameter
gradients that arrive by float atomics are held to the bound tests/test_hip_mlp_pack.py uses for them.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_hip_mlp import OUT_RANGE, _pack, _warp_params, _warp_ref
from tests.test_hip_mlp_pack import PAD, SCALES, SENT, _atomic_close, _engine, _fenced, _intact, _params

gpu = pytest.mark.gpu
DEV = 'cuda'
CASES = ((0, 40), (1, 1), (17, 40), (4096, 4096), (54613, 54613))      # (count, capacity): one capacity above the count, count = 0
W_OFF = [0, 512, 512 + 16512, 512 + 2 * 16512, 512 + 3 * 16512]        # W0 b0 | W1 b1 | W2 b2 | W3 b3 | W4 b4
W_SHAPE = [(128, 3), (128, 128), (128, 128), (128, 128), (4, 128)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), f'{what}: differs in {int((_bits(a) != _bits(b)).sum())} of {a.numel()} entries'


def _inputs(M, cap):
    g = torch.Generator().manual_seed(M + 1)
    pts = (torch.randn(cap, 3, generator=g) * 0.5).to(DEV)
    og = torch.randn(cap, 16, generator=g).to(DEV)
    return pts, og, torch.tensor([M], dtype=torch.int32, device=DEV)


def _run(params, M, cap, ctx, lean, staged=False, bufs=None):
    """One forward + backward pass of the warp net in sentinel-fenced buffers; lean: inside a scope opened for these buffers
    (bufs: buffers of the caller's instead of fresh ones)."""
    from poseprobe_amd import ops
    pts, og, count = _inputs(M, cap)
    na, ns = 4 * cap * 4 * 128, 3 * cap * 4 * 128 + 49152
    arenas = bufs or {k: _fenced(n) for k, n in (('acts', na), ('scratch', ns), ('pgrad', params.numel()), ('pts_grad', cap * 3),
                                                 ('out', cap * 16))}
    acts, scratch, pgrad, ptsg, out = (arenas[k][1] for k in ('acts', 'scratch', 'pgrad', 'pts_grad', 'out'))
    pgrad.zero_()
    ptsg.fill_(0.25)
    if lean:
        ops.warp_lean_begin(acts, scratch, params, ctx)
    ops.warp_fwd(params, pts, count, cap, OUT_RANGE, acts, out, ctx)
    if staged:
        stage2 = ops.warp_bwd_data(params, pts, acts, og, count, cap, OUT_RANGE, scratch, pgrad, ptsg, ctx)
        ops.warp_bwd_weights(acts, scratch, count, cap, pgrad, stage2, ctx)
    else:
        ops.warp_bwd(params, pts, acts, og, count, cap, OUT_RANGE, scratch, pgrad, ptsg, ctx)
    if lean:
        ops.warp_lean_end(ctx)
    torch.cuda.synchronize()
    for k, (arena, view) in arenas.items():
        _intact(arena, view.numel(), f'{k} (M = {M}, capacity {cap}, lean = {lean}, staged = {staged})')
    return dict(out=out, acts=acts.view(4, cap * 4, 128), scratch=scratch, pts_grad=ptsg, pgrad=pgrad, og=og)


@functools.lru_cache(maxsize=4)
def _float64_grads(M, cap, scale):
    """Parameter gradients of the same network and inputs in float64 (autograd on tests/test_hip_mlp.py's restatement)."""
    if M == 0:
        return None
    pts, og, _ = _inputs(M, cap)
    lay = [((W * scale).double().to(DEV).requires_grad_(True), (b * scale).double().to(DEV).requires_grad_(True))
           for W, b in _warp_params(3)]
    ref = _warp_ref(lay, pts[:M].double())
    (ref.reshape(M, 16) * og[:M].double()).sum().backward()
    return [(W.grad, b.grad) for W, b in lay]


def _errors(pgrad, ref):
    """relative rms error of every weight and bias gradient against `ref`."""
    e = []
    for (gW, gb), off, (o, k) in zip(ref, W_OFF, W_SHAPE):
        for got, want in ((pgrad[off:off + o * k].view(o, k).double(), gW), (pgrad[off + o * k:off + o * k + o].double(), gb)):
            den = float((want ** 2).mean().sqrt())
            e.append(float(((got - want) ** 2).mean().sqrt()) / den if den > 0 else float((got != 0).any()))
    return e


def _check_lean_against_full(lean, full, M, cap, what):
    # forward: out, X1 .. X3 and the primal rows of X0 bit for bit; the tangent rows of X0 untouched (the full form writes them)
    _same(lean['out'], full['out'], f'{what}: out')
    _same(lean['acts'][1:], full['acts'][1:], f'{what}: X1 .. X3')
    _same(lean['acts'][0, 0::4], full['acts'][0, 0::4], f'{what}: primal rows of X0')
    tang = torch.ones(cap * 4, dtype=torch.bool, device=DEV)
    tang[0::4] = False
    assert bool((_bits(lean['acts'][0, tang]) == SENT).all()), f'{what}: tangent rows of X0 were written in lean form'
    if M > 0:
        assert bool((_bits(full['acts'][0, :4 * M][tang[:4 * M]]) != SENT).all()), f'{what}: the full form did not write X0'
    # data gradients: pts_grad, Ybar2, Ybar1 bit for bit; slot 0 = out_range * out_grad in its first 16 M floats, untouched behind
    _same(lean['pts_grad'], full['pts_grad'], f'{what}: pts_grad')
    LS = cap * 4 * 128
    _same(lean['scratch'][LS:], full['scratch'][LS:], f'{what}: Ybar2, Ybar1 (and the tail of scratch)')
    _same(lean['scratch'][:16 * M], (lean['og'][:M] * OUT_RANGE).reshape(-1), f'{what}: scaled output gradients in slot 0')
    assert bool((_bits(lean['scratch'][16 * M:LS]) == SENT).all()), f'{what}: slot 0 behind the output gradients was written'
    _atomic_close(lean['pgrad'], full['pgrad'], f'{what}: parameter gradients, lean against full')


NAMES = [f'{t}{i}' for i in range(5) for t in ('W', 'b')]
HIDDEN = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')                             # what the weight-gradient kernel produces


def _assert_as_accurate(ef, el, M, names, what):
    """the rule of tests/test_hip_wgrad_split.py: 1.25 x the full form's miss of float64 (1.5 x from 100 k rows up, where a
    work-group's fp32 sums are long), with its floor of 4e-7 for sums of few rows, where fp32 rounds once"""
    ratio = 1.5 if 4 * M >= 100000 else 1.25
    for n, a, b in zip(NAMES, ef, el):
        if n in names:
            assert b <= ratio * a + 1e-9 or b <= 4e-7, f'{what}: {n} misses float64 by {b:.3e}, the full form by {a:.3e}'


@gpu
@pytest.mark.parametrize('pack', [1, 0])
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('M,cap', CASES)
def test_lean_pass_against_full_pass(M, cap, scale, pack):
    """Forward, data gradients and weight gradients of one pass, one-shot and staged, lean against full on the same inputs; the
    parameter gradients of both against float64: a lean result may miss the float64 gradient by at most 1.25 x the full form's miss.
    Twice: with float atomics, for W1 .. W3 and b1 .. b3 (the weight-gradient kernel's, which the lean form computes differently),
    and with the ordered flush attached for all ten tensors.  The thin layers' gradients (W0, b0, W4, b4) come from the same
    arithmetic in both forms and differ only by the arrival order of their float atomics - which moves b4's miss between 1.9e-7
    and 5.8e-7 from one run to the next of the SAME kernel at 54 613 samples, more than the rule allows between the two forms; with
    the order fixed they must be equal bit for bit."""
    from poseprobe_amd import ops
    warp, rgbp = _params(scale)
    what = f'M = {M}, capacity {cap}, weights x {scale}, mlp_pack = {pack}'
    ref = _float64_grads(M, cap, scale)
    wgs = torch.cuda.get_device_properties(DEV).multi_processor_count
    for ordered in (False, True):
        ctx = ops.Context(mlp_pack=pack)
        if ordered:
            work = torch.empty(ops.ordered_workspace(wgs, cap, 64), dtype=torch.uint8, device=DEV)
            ops.ordered_attach(ctx, work, wgs, cap, 64)
        packbuf = torch.empty(ops.mlp_pack_workspace(), device=DEV)
        ops.mlp_pack(warp, rgbp, packbuf, ctx)
        tag = what + (', ordered flush' if ordered else ', float atomics')
        full = _run(warp, M, cap, ctx, lean=False)
        lean = _run(warp, M, cap, ctx, lean=True)
        staged = _run(warp, M, cap, ctx, lean=True, staged=True)
        ops.mlp_pack_invalidate(ctx)
        _check_lean_against_full(lean, full, M, cap, tag + ', one-shot')
        _check_lean_against_full(staged, full, M, cap, tag + ', staged')
        for k in ('out', 'acts', 'scratch', 'pts_grad'):
            _same(lean[k], staged[k], f'{tag}: {k}, one-shot against staged')
        _atomic_close(lean['pgrad'], staged['pgrad'], f'{tag}: parameter gradients, one-shot against staged')
        if ordered:
            _same(lean['pgrad'], staged['pgrad'], f'{tag}: parameter gradients, one-shot against staged')
            for off, (o, k) in ((W_OFF[0], W_SHAPE[0]), (W_OFF[4], W_SHAPE[4])):
                _same(lean['pgrad'][off:off + o * k + o], full['pgrad'][off:off + o * k + o], f'{tag}: thin-layer gradients at {off}')
        if ref is None:
            assert float(lean['pgrad'].abs().max()) == 0 and float(staged['pgrad'].abs().max()) == 0
            continue
        ef = _errors(full['pgrad'], ref)
        for run, form in ((lean, 'one-shot'), (staged, 'staged')):
            el = _errors(run['pgrad'], ref)
            print(f'{tag}, {form}: ' + ', '.join(f'{n} full {a:.3e} lean {b:.3e}' for n, a, b in zip(NAMES, ef, el)))
            _assert_as_accurate(ef, el, M, NAMES if ordered else HIDDEN, f'{tag}, {form}')


@gpu
@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('M', [1, 17, 32])
def test_lean_gradients_do_not_depend_on_the_pack_at_two_work_groups(M, scale):
    """At most two work-groups add to every entry (a + b is commutative): pack on and pack off agree bit for bit in lean form."""
    from poseprobe_amd import ops
    warp, rgbp = _params(scale)
    res = []
    for pack in (1, 0):
        ctx = ops.Context(mlp_pack=pack)
        packbuf = torch.empty(ops.mlp_pack_workspace(), device=DEV)
        ops.mlp_pack(warp, rgbp, packbuf, ctx)
        res.append(_run(warp, M, M, ctx, lean=True))
        ops.mlp_pack_invalidate(ctx)
    for k in ('out', 'acts', 'scratch', 'pts_grad', 'pgrad'):
        _same(res[0][k], res[1][k], f'M = {M}, weights x {scale}: {k}, mlp_pack = 1 against 0 in lean form')


@gpu
def test_only_the_recorded_context_and_buffers_take_the_lean_form():
    from poseprobe_amd import ops
    M = cap = 1000
    warp, _ = _params(0.09)
    ctx, other = ops.Context(), ops.Context()
    full = _run(warp, M, cap, ctx, lean=False)
    na, ns = 4 * cap * 4 * 128, 3 * cap * 4 * 128 + 49152
    rec_acts, rec_scratch = _fenced(na)[1], _fenced(ns)[1]

    def same_as_full(r, what):
        for k in ('out', 'acts', 'pts_grad'):
            _same(r[k], full[k], f'{what}: {k}')
        _same(r['scratch'][:3 * cap * 4 * 128], full['scratch'][:3 * cap * 4 * 128], f'{what}: Ybar3, Ybar2, Ybar1')
        _atomic_close(r['pgrad'], full['pgrad'], f'{what}: parameter gradients')

    ops.warp_lean_begin(rec_acts, rec_scratch, warp, ctx)
    same_as_full(_run(warp, M, cap, ctx, lean=False), 'other buffers inside an open scope')
    same_as_full(_run(warp, M, cap, ctx, lean=False, staged=True), 'other buffers inside an open scope, staged')
    # the recorded buffers, but through another context
    arenas = {k: _fenced(n) for k, n in (('acts', na), ('scratch', ns), ('pgrad', warp.numel()), ('pts_grad', cap * 3), ('out', cap * 16))}
    ops.warp_lean_begin(arenas['acts'][1], arenas['scratch'][1], warp, ctx)
    same_as_full(_run(warp, M, cap, other, lean=False, bufs=arenas), 'recorded buffers through another context')
    # ... and through the recording context: lean (the scope is still open)
    for k in ('acts', 'scratch'):
        _bits(arenas[k][1]).fill_(SENT)
    lean = _run(warp, M, cap, ctx, lean=False, bufs=arenas)
    assert bool((_bits(lean['scratch'][16 * M:cap * 4 * 128]) == SENT).all()), 'recorded buffers, recording context: Ybar3 was written'
    assert bool((_bits(lean['acts'][0, 1::4]) == SENT).all()), 'recorded buffers, recording context: tangent rows of X0 were written'
    _same(lean['scratch'][:16 * M], (lean['og'][:M] * OUT_RANGE).reshape(-1), 'recorded buffers, recording context: slot 0')
    _atomic_close(lean['pgrad'], full['pgrad'], 'recorded buffers, recording context: parameter gradients')
    ops.warp_lean_end(ctx)
    for k in ('acts', 'scratch'):
        _bits(arenas[k][1]).fill_(SENT)
    after = _run(warp, M, cap, ctx, lean=False, bufs=arenas)
    same_as_full(after, 'recorded buffers after the end of the scope')
    assert bool((_bits(after['acts'][:, :4 * M]) != SENT).all()), 'after the end of the scope: not all of acts was written'
    # an option that takes a kernel off the split-precision path: nothing is recorded
    for opts in ({'warp_lean': 0}, {'mlp_split': 31 & ~16}, {'mlp_split': 31 & ~1}, {'mlp_split': 31 & ~2}, {'mlp_fused': 0}):
        cx = ops.Context(**opts)
        same = _run(warp, M, cap, cx, lean=True)
        ref = _run(warp, M, cap, cx, lean=False)
        for k in ('out', 'acts', 'pts_grad'):
            _same(same[k], ref[k], f'{opts}: {k}')
        _same(same['scratch'][:3 * cap * 4 * 128], ref['scratch'][:3 * cap * 4 * 128], f'{opts}: scratch')


@gpu
def test_weight_gradient_stage_on_foreign_operands_inside_a_scope():
    """pp_warp_bwd_weights on random X and Y that no forward pass produced (tests/test_hip_wgrad_split.py), while a scope is open
    for other buffers: Ybar^T X of exactly these operands, which are not written."""
    from poseprobe_amd import ops
    from tests.test_hip_wgrad_split import _layout, _operands
    M, cap = 4099, 4099
    g = torch.Generator().manual_seed(5)
    Y, X, acts, scratch, _ = _operands('warp', M, cap, g)
    acts0, scratch0 = acts.clone(), scratch.clone()
    _, _, _, npg, layers = _layout('warp', cap)
    count = torch.tensor([M], dtype=torch.int32, device=DEV)
    ctx = ops.Context()
    warp, _ = _params(0.09)
    ops.warp_lean_begin(torch.zeros_like(acts), torch.zeros_like(scratch), warp, ctx)
    grad = torch.zeros(npg, device=DEV)
    ops.warp_bwd_weights(acts, scratch, count, cap, grad, 1, ctx)
    ops.warp_lean_end(ctx)
    torch.cuda.synchronize()
    assert torch.equal(acts, acts0) and torch.equal(scratch, scratch0), 'operands were written'
    for i, (off, kx) in enumerate(layers):
        ref = Y[i].to(DEV).double().T @ X[i].to(DEV).double()
        got = grad[off:off + 128 * kx].view(128, kx).double()
        err = float(((got - ref) ** 2).mean().sqrt()) / float((ref ** 2).mean().sqrt())
        assert err < 5e-6, f'layer {i}: relative rms error {err:.3e} against float64 of the given operands'


@gpu
def test_engine_step_with_and_without_the_lean_scope():
    """Two engines from one state, option warp_lean 1 and 0, one render_and_grads: everything the data path produces is equal bit
    for bit, the parameter gradients within the bound of float atomics - and the lean engine did run lean."""
    from poseprobe_amd import synthetic as syn
    a, (npix, N) = _engine({'warp_lean': 1})
    b, _ = _engine({'warp_lean': 0})
    assert a.ctx.get('warp_lean') == 1 and b.ctx.get('warp_lean') == 0
    idx, jit = syn.step_randomness(npix, N, seed=1)
    for e in (a, b):
        e.zero_grads()
        e.render_and_grads(torch.tensor(idx, dtype=torch.int32, device='cuda:0'), torch.tensor(jit, device='cuda:0'), 10)
    torch.cuda.synchronize()
    M = int(a.ws.count.item())
    assert M == int(b.ws.count.item()) and M > 0
    for name in ('warp_out', 'rgb', 'g_warp_out', 'g_pts'):
        _same(getattr(a.ws, name)[:M], getattr(b.ws, name)[:M], f'engine step: {name}')
    _same(a.ws.rgb_marched, b.ws.rgb_marched, 'engine step: rgb_marched')
    _atomic_close(a.flat.grad, b.flat.grad, 'engine step: flat parameter gradients')
    LS = a.ws.cap * 4 * 128
    assert float(a.ws.scratch[16 * M:LS].abs().max()) == 0 and float(b.ws.scratch[16 * M:4 * M * 128].abs().max()) > 0
    _same(a.ws.scratch[:16 * M], (a.ws.g_warp_out[:M] * float(a.cfg.out_range)).reshape(-1), 'engine step: slot 0 of scratch')


@gpu
def test_deterministic_engine_stays_bit_reproducible():
    """TrainEngine(deterministic=True) opens the lean scope as well (the ordered flush of the weight-gradient kernel is the full
    form's): two runs from one state are equal bit for bit in every state tensor."""
    from tests.test_hip_deterministic import assert_same_bits, run_small
    opts = {'mlp_fused': 1, 'mlp_split': 31}                   # what deterministic=True needs, whatever the default context was seeded with
    a, b = run_small(3, deterministic=True, options=opts), run_small(3, deterministic=True, options=opts)
    for s, (x, y) in enumerate(zip(a, b)):
        assert_same_bits(x, y, f'step {s + 1}')


def test_option_is_listed_and_defaults_to_on():
    from poseprobe_amd import _lib
    assert 'warp_lean' in _lib.OPTION_NAMES and _lib.library_default('warp_lean') == 1
    assert _lib.Context().get('warp_lean') == 1
