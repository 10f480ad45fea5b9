"""GPU tests of the optimiser and total-variation kernels (csrc/pp_optim.hip, k_grid_tv_grad of csrc/pp_grid.hip) against the
float64 references of tests/optim_reference.py.

Cases, inputs and tolerances live in tests/optim_cases.py.  Every element has to meet the tolerance: the sign of a difference of
two float32 numbers is exact and Adam is smooth in everything else, parameters are 0.1 * randn (no difference near the denormal
range) and the exact ties are planted by copying values - across every x border (so across every chunk border, every slab border
and into the last plane) and in y and z on every plane.  Each tolerance is 4 x the error a float32 evaluation of the reference
makes on the same inputs (tests/test_optim_reference.py re-measures it); every comparison prints the kernel's own error in the
same unit.
"""
import pytest
import torch

from tests import optim_cases as K
from tests import optim_reference as R
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

ADAM = (K.B1, K.B2, K.EPS)


def close(kind, a, ref, what):
    print(f'{what}: {kind} kernel error {K.measured(a, ref, kind):.3e} (tolerance {sum(K.TOL[kind].values()):.0e})')
    assert_close(a, ref, atol=0.0, name=f'{what} {kind}', **K.TOL[kind])


def same_bits(a, b, what):
    assert torch.equal(a.cpu(), b.cpu()), f'{what}: {int((a.cpu() != b.cpu()).sum())} of {a.numel()} entries differ'


def planes(X, slabs):
    inside = torch.zeros(X, dtype=torch.bool)
    for xb, xe in slabs:
        inside[xb:xe] = True
    return inside


def check_grid_result(what, ref, inputs, out, inside, tv_complete=False):
    """out = (p_in, p_out, grad, m, v, tv or None) after the kernel, inputs = (p, grad, m, v) before it, ref = (p_out, m, v,
    grad, tv) in float64.  Inside the slab(s): the reference within tolerance.  Outside: p_out still the canary, both moments and
    the gradient bit-identical to what they held; p_in unchanged everywhere."""
    p, grad, m, v = inputs
    d_p, d_po, d_g, d_m, d_v, d_tv = (None if t is None else t.cpu() for t in out)
    same_bits(d_p, p, f'{what} p_in')
    assert bool((d_po[~inside] == K.CANARY).all()), f'{what}: p_out written outside the slab'
    same_bits(d_m[~inside], m[~inside], f'{what} m outside the slab')
    same_bits(d_v[~inside], v[~inside], f'{what} v outside the slab')
    same_bits(d_g[~inside], grad[~inside], f'{what} grad outside the slab')
    close('grid.p', d_po[inside], ref[0][inside], what)
    close('grid.m', d_m[inside], ref[1][inside], what)
    close('grid.v', d_v[inside], ref[2][inside], what)
    same_bits(d_g[inside].double(), ref[3][inside], f'{what} grad inside the slab')
    if d_tv is not None:
        close('grid.tv', d_tv[0], ref[4], what)
        if tv_complete:
            close('grid.tv', d_tv[0], R.tv_value(p), what + ' (slabs add up to the grid)')


# ------------------------------------------------------------------------------------------------------- fused pass, dense
@pytest.mark.parametrize('case,hyper', K.dense_params(), ids=[f'{c[0]}-{h[0]}' for c, h in K.dense_params()])
def test_fused_pass_dense(case, hyper):
    """pp_grid_tv_adam_step slab after slab on one set of buffers; the reason of each shape stands in optim_cases.DENSE_CASES."""
    from poseprobe_amd import ops
    what, shape, slabs, _ = case
    _, step, grad_scale, tv_scale, lr, with_tv = hyper
    X, Y, Z, C = shape
    inputs = K.grid_inputs(shape)
    ref = K.reference_dense(shape, slabs, hyper)
    d_p, d_g, d_m, d_v = (t.cuda() for t in inputs)
    d_po = torch.full_like(d_p, K.CANARY)
    d_tv = torch.zeros(1, device='cuda') if with_tv else None
    for xb, xe in slabs:
        ops.grid_tv_adam_step(d_p, d_po, d_g, d_m, d_v, (X, Y, Z), C, xb, xe, tv_scale, grad_scale, lr, *ADAM, step, d_tv)
    inside = planes(X, slabs)
    check_grid_result(what, ref, inputs, (d_p, d_po, d_g, d_m, d_v, d_tv), inside, tv_complete=bool(inside.all()))
    if lr == 0:
        same_bits(d_po.cpu()[inside], inputs[0][inside], 'lr = 0: p_out inside the slab')
        assert not torch.equal(d_m.cpu()[inside], inputs[2][inside]) and not torch.equal(d_v.cpu()[inside], inputs[3][inside])
    if tv_scale == 0:       # a voxel with grad = m = v = 0 then has an exactly zero gradient: nothing of it may move
        p, grad, m, v = inputs
        still = ((grad == 0).all(-1) & (m == 0).all(-1) & (v == 0).all(-1))
        still[~inside] = False
        assert bool(still.any())
        same_bits(d_po.cpu()[still], p[still], 'zero voxel p')
        assert float(d_m.cpu()[still].abs().max()) == 0.0 and float(d_v.cpu()[still].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- option grid_chunks
def test_grid_chunks_option_changes_the_cut_and_nothing_else():
    """Context(grid_chunks=k): 1, 3 and 11 chunks (chunk lengths 11, 4 with a last chunk of 3, and 1) on an interior slab of 11
    planes; 12 and 4096 exceed the slab and behave as 0 (the heuristic: 6 chunks of 2, the last of 1).  p_out, both moments and
    the gradient are bit-identical for every k and equal the reference; the TV value is the same sum in another order."""
    from poseprobe_amd import _lib, ops
    shape, (xb, xe) = K.CHUNK_CASE
    X, Y, Z, C = shape
    inputs = K.grid_inputs(shape)
    hyper = ('chunks', 3, 0.5, K.TV_SCALE, K.LR, True)
    ref = K.reference_dense(shape, [(xb, xe)], hyper)
    inside = planes(X, [(xb, xe)])
    first = None
    for k in K.CHUNK_VALUES:
        ctx = _lib.Context(grid_chunks=k)
        assert ctx.get('grid_chunks') == k
        d_p, d_g, d_m, d_v = (t.cuda() for t in inputs)
        d_po = torch.full_like(d_p, K.CANARY)
        d_tv = torch.zeros(1, device='cuda')
        ops.grid_tv_adam_step(d_p, d_po, d_g, d_m, d_v, (X, Y, Z), C, xb, xe, K.TV_SCALE, 0.5, K.LR, *ADAM, 3, d_tv, ctx=ctx)
        out = (d_p, d_po, d_g, d_m, d_v, d_tv)
        check_grid_result(f'grid_chunks={k}', ref, inputs, out, inside)
        if first is None:
            first = [t.cpu() for t in out[1:5]]
        for a, b, name in zip(first, out[1:5], ('p_out', 'grad', 'm', 'v')):
            same_bits(a, b, f'grid_chunks={k} against grid_chunks={K.CHUNK_VALUES[0]}: {name}')


# ------------------------------------------------------------------------------------------------------ fused pass, sparse
@pytest.mark.parametrize('case', K.SPARSE_CASES, ids=[c[0] for c in K.SPARSE_CASES])
def test_fused_pass_sparse(case):
    """pp_grid_tv_adam_step_sparse with a map marking ~10 % of the voxels (first and last plane of the slab included, one marked
    voxel with a zero gradient, unmarked voxels with non-zero gradients): the reference with the same map inside the slab, the
    unmarked gradients bit-unchanged, the other map cleared inside the slab only, the map itself unchanged; with every voxel
    marked, the dense call bit for bit."""
    from poseprobe_amd import ops
    what, shape, (xb, xe), _ = case
    X, Y, Z, C = shape
    p, grad, m, v, hit = K.sparse_inputs(shape, (xb, xe))
    inputs = (p, grad, m, v)
    a = (xb, xe, K.TV_SCALE, 0.5, K.LR, *ADAM, 3)
    ref = R.grid_step(p, grad, m, v, *a, touched=hit)
    inside = planes(X, [(xb, xe)])

    def run(touched, dense=False):
        d_p, d_g, d_m, d_v = (t.cuda() for t in inputs)
        d_po = torch.full_like(d_p, K.CANARY)
        d_tv = torch.zeros(1, device='cuda')
        stale = torch.ones(X, Y, Z, dtype=torch.uint8, device='cuda')
        if dense:
            ops.grid_tv_adam_step(d_p, d_po, d_g, d_m, d_v, (X, Y, Z), C, *a, d_tv)
        else:
            ops.grid_tv_adam_step_sparse(d_p, d_po, d_g, d_m, d_v, (X, Y, Z), C, *a, d_tv, touched, stale)
        return (d_p, d_po, d_g, d_m, d_v, d_tv), stale.cpu()

    d_hit = hit.cuda()
    out, stale = run(d_hit)
    check_grid_result(what, ref, inputs, out, inside)
    unmarked = (hit == 0) & inside[:, None, None]
    assert float(grad[unmarked].abs().max()) > 0
    same_bits(out[2].cpu()[unmarked], grad[unmarked], 'gradient of the unmarked voxels')
    assert int(stale[inside].sum()) == 0, 'touched_clear not cleared inside the slab'
    assert bool((stale[~inside] == 1).all()), 'touched_clear written outside the slab'
    same_bits(d_hit, hit, 'touched map')
    full, stale = run(torch.ones(X, Y, Z, dtype=torch.uint8, device='cuda'))
    dense, _ = run(None, dense=True)
    for x, y, name in zip(full[1:5], dense[1:5], ('p_out', 'grad', 'm', 'v')):
        same_bits(x, y, f'{what}: every voxel marked against the dense call: {name}')
    close('grid.tv', full[5].cpu()[0], dense[5].cpu()[0].double(), what + ' every voxel marked')
    assert int(stale[inside].sum()) == 0 and bool((stale[~inside] == 1).all())


# ------------------------------------------------------------------------------------------- pp_grid_tv_value / pp_grid_tv_grad
TV_VALUE_SHAPES = [(s, 'dense shape, whole grid') for s in K.TV_SHAPES] + [(c[1], c[2]) for c in K.TV_VALUE_ONLY]


@pytest.mark.parametrize('shape', [s for s, _ in TV_VALUE_SHAPES], ids=['x'.join(map(str, s)) for s, _ in TV_VALUE_SHAPES])
def test_tv_value(shape):
    """out += sum |forward differences|: accumulated onto a non-zero start, p unchanged.  At 8x105x105x12 the pass has more
    (tile, chunk) pairs (130 x 8 = 1040) than work-groups (1024): tiles 128 and 129, 0.9 % of every plane, are reached by the
    second pass of the persistent loop only; its 1024 float atomics make the result a serial float32 sum of as many partials,
    which is what that shape is measured against (optim_cases.serial_partial_sums)."""
    from poseprobe_amd import ops
    X, Y, Z, C = shape
    p = K.tv_inputs(shape)[0]
    d_p = p.cuda()
    out = torch.zeros(1, device='cuda')
    ops.grid_tv_value(d_p, (X, Y, Z), C, out)
    ref = R.tv_value(p)
    kind = 'tv.value.serial' if shape in [c[1] for c in K.TV_VALUE_ONLY] else 'tv.value'
    close(kind, out.cpu()[0], ref, 'tv value')
    ops.grid_tv_value(d_p, (X, Y, Z), C, out)
    close(kind, out.cpu()[0], 2 * ref, 'tv value accumulated twice')
    same_bits(d_p, p, 'p')


@pytest.mark.parametrize('shape', K.TV_SHAPES + K.TV_ELEMENTWISE, ids=lambda s: 'x'.join(map(str, s)))
def test_tv_grad(shape):
    """grad += scale * g_scalar[0] * d tv_value / d p onto a non-zero gradient; C = 1, 3, 5 take the element-wise kernel.  A
    g_scalar of 0 leaves the gradient bit-unchanged."""
    from poseprobe_amd import ops
    X, Y, Z, C = shape
    p, g0 = K.tv_inputs(shape)
    d_p, d_g = p.cuda(), g0.cuda()
    ops.grid_tv_grad(d_p, (X, Y, Z), C, K.TV_SCALE_ARG, torch.full((1,), K.TV_GSCALAR, device='cuda'), d_g)
    close('tv.grad', d_g.cpu(), g0.double() + K.TV_SCALE_ARG * K.TV_GSCALAR * R.tv_grad(p), 'tv grad')
    same_bits(d_p, p, 'p')
    d_g = g0.cuda()
    ops.grid_tv_grad(d_p, (X, Y, Z), C, K.TV_SCALE_ARG, torch.zeros(1, device='cuda'), d_g)
    same_bits(d_g, g0, 'gradient after g_scalar = 0')


def test_tv_value_refuses_channel_counts_the_gradient_accepts():
    """pp_grid_tv_grad serves any channel count (element-wise kernel), pp_grid_tv_value only multiples of 4: pinned as it is."""
    from poseprobe_amd import ops
    from poseprobe_amd._lib import PoseProbeError
    p = K.tv_inputs((5, 6, 7, 1))[0].cuda()
    out = torch.full((1,), 3.5, device='cuda')
    with pytest.raises(PoseProbeError):
        ops.grid_tv_value(p, (5, 6, 7), 1, out)
    torch.cuda.synchronize()
    assert float(out[0]) == 3.5


# ------------------------------------------------------------------------------------------------------------ pp_adam_flat
@pytest.mark.parametrize('hyper', K.FLAT_HYPER, ids=lambda h: f'gscale{h[0]}-zero{h[1]}-step{h[2]}')
@pytest.mark.parametrize('n', K.FLAT_N)
def test_adam_flat(n, hyper):
    """Three consecutive steps (the moments carry over).  n = 1, 255, 256, 257: the tail of a 256-thread block; n = 1000: five
    segments with ends {1, 256, 257, 700, 900} - one element, an end on a block border, a frozen segment (lr = 0: p bit-unchanged,
    moments updated), a last end short of n (the rest takes the last rate).  Compared segment by segment, each against its own
    largest entry."""
    from poseprobe_amd import ops
    grad_scale, zero_grad, step0 = hyper
    seg_end, seg_lr = K.flat_segments(n)
    p, m, v, grads = K.flat_inputs(n)
    ref = K.reference_flat(n, hyper)
    d_p, d_m, d_v = p.cuda(), m.cuda(), v.cuda()
    d_end = torch.tensor(seg_end, dtype=torch.int32, device='cuda')
    d_lr = torch.tensor(seg_lr, dtype=torch.float32, device='cuda')
    before = p
    for s in range(K.FLAT_STEPS):
        d_g = grads[s].cuda()
        ops.adam_flat(d_p, d_g, d_m, d_v, d_end, d_lr, grad_scale, *ADAM, step0 + s, zero_grad)
        same_bits(d_g.double(), ref[s][3], f'step {step0 + s}: gradient {"zeroed" if zero_grad else "kept"}')
        for sl, lr in zip(K.flat_segment_slices(n), seg_lr):
            what = f'n={n} step {step0 + s} segment [{sl.start},{sl.stop}) lr={lr:g}'
            close('flat.p', d_p.cpu()[sl], ref[s][0][sl], what)
            close('flat.m', d_m.cpu()[sl], ref[s][1][sl], what)
            close('flat.v', d_v.cpu()[sl], ref[s][2][sl], what)
            if lr == 0:
                same_bits(d_p.cpu()[sl], before[sl], what + ': frozen p')
    same_bits(d_end, torch.tensor(seg_end, dtype=torch.int32), 'seg_end')
