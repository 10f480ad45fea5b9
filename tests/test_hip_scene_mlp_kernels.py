"""The scene branch's MLP chain (csrc/pp_nerf.hip, pp_nerf_trunk.h, pp_gemm*.h, pp_gemm_tn_tr.h: pp_nerf_fwd / pp_nerf_bwd through
ops.nerf_fwd / ops.nerf_bwd) stage by stage against float64, on its three routes: fused (nerf_split = 1, nerf_chain = 3, the
default), layer by layer with split precision (nerf_chain = 0) and layer by layer on the fp32 matrix instructions (nerf_split = 0).

A pass leaves every intermediate in its two blocks (tests/scene_mlp_reference.py restates their layouts), so each stage - the eight
feature layers, the density head, the colour head's two layers, dH, the heads' parameter gradients, dHsum, dView, the density column
of d7, d7, DY[6 .. 0], the nine weight-gradient products with their bias sums, dEncS, dEnc0, g_center / g_ray - is compared with
a float64 evaluation of that stage alone on the kernel's own stored inputs and ReLU states.  Assertions, and no other tolerance:
  * helpers.check at its default:  |hip - ref64| <= 2 |ref32 - ref64| + 8 eps32 * scale  on every entry of every stage;
  * np.array_equal / == for the exact promises: the mask planes are (own stored activation > 0) in the layout of the route, the
    skip copy of the encoding, the zero columns 257 .. 287 of d7, the zero gradients of the padding columns, and - no upstream
    gradient - exactly zero gradients;
  * 4096 sentinel floats behind rgb_samples, density_samples, g_center, g_ray and params_grad come back unchanged.
Seeded inputs: tests/scene_mlp_cases.py (three band schedules, bd in {0.1, 20, -30}, ray lengths 1e-3 .. 10); the references are tied
to oracle.scene_nerf by tests/test_scene_mlp_reference.py.  The two device-derived sizes (a second tile per work-group of the fused
chain and of the persistent GEMMs; a second 256-row strip per work-group of the heads' backward kernels) run once, on the default
route, with the float64 references evaluated by torch on the device; their row-independent stages are compared on the first two
tiles, the last two and the first two of the second round.

ulps each stage needed on each route when these tests were written (a record, not a bound: the bound stays 8): DESIGN.md, section 5.

One-line value mutations of the kernels these tests were tried against (none moves an address or a bound), each failing
test_every_stage_against_float64 at 4x64 and 29x67 unless another test is named:
  layer 4's skip columns from enc column j - 1, in the fused chain's tile load (a4, fused) and in k_nerf_encode's copy (the exact
  skip-copy promise on every route, a4 on the fused one);  the data-gradient mask of layer l instead of l - 1 (DY6 fused, DY5
  layer by layer);  the density column left out of d7 -> DY6, as d = 0 in the fused epilogue and as a zero column of W7^T (DY6);
  softplus' with 0 in its > 20 branch (d7[:,256] at bd = 20);  k_nerf_ray_sum from s = q + 4 (dHsum);  k_nerf_part_finish over
  rows - 1 rows (g.R1);  the strip loop of k_nerf_rgb_bwd / k_nerf_density_bwd doing its first strip only
  (test_second_round_sizes_on_the_default_route[second_strip]: dH; the density column of d7 keeps its prefill);  dEncS omitted in
  k_nerf_encode_bwd (g_center);  the sign of the cosine term of the view path (g_ray).
One mutation changes no float32 value and is therefore caught by nothing: softplus' WITHOUT its > 20 branch.  For x > 20,
expf(-x) < 2.1e-9 is below half an ulp of 1, so 1 / (1 + expf(-x)) is exactly 1.0f, the value of the branch.
"""
import pytest
import torch

from tests import scene_mlp_cases as C
from tests import scene_mlp_reference as MR
from tests.helpers import check, cu

pytestmark = pytest.mark.gpu

ROUTES = {'fused': dict(nerf_split=1, nerf_chain=3), 'layered': dict(nerf_split=1, nerf_chain=0), 'fp32': dict(nerf_split=0)}
GUARD, SENT = 4096, 0x7FC0DEAD                              # a quiet-NaN payload no kernel produces
_CTX = {}
SINGLE_TERM_DY6 = 88                                        # ulps: twice the 44.33 measured on an MI355X; see test_missing_upstream_gradients


def context(route):
    from poseprobe_amd import ops
    if route not in _CTX:
        _CTX[route] = None if route == 'default' else ops.Context(**ROUTES[route])
    return _CTX[route]


def guarded(n, fill):
    buf = torch.empty(n + GUARD, dtype=torch.int32, device='cuda').fill_(SENT).view(torch.float32)
    buf[:n] = fill
    return buf


def untouched(what, buf, n):
    assert bool((buf[n:].view(torch.int32) == SENT).all()), f'{what}: the sentinels behind the buffer were overwritten'


def run_pass(c, route, ordered=False):
    """One pp_nerf_fwd + pp_nerf_bwd on the case `c` -> scene_mlp_reference.make_run of what they read and left (device tensors)."""
    from poseprobe_amd import ops
    ctx = context(route)
    R, S = c['depth'].shape
    M = R * S
    flat, center, ray, depth, bands, g_rgb, g_den = (cu(c[k]) for k in ('flat', 'center', 'ray', 'depth', 'bands', 'g_rgb', 'g_den'))
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    n_acts, n_scr = ops.nerf_workspace(M, R)
    assert (n_acts, n_scr) == MR.workspace_floats(M, R)
    acts, scr = torch.zeros(n_acts, device='cuda'), torch.zeros(n_scr, device='cuda')
    scr[:M * 320] = float('nan')                           # d7's block: its zero columns 257 .. 287 have to be WRITTEN
    nan = float('nan')
    rgb_s, dens, gc, gr = guarded(M * 3, nan), guarded(M, nan), guarded(R * 3, nan), guarded(R * 3, nan)
    grad = guarded(flat.numel(), 0.0)                      # params_grad is accumulated into: zeroed first
    ops.nerf_fwd(flat, center, ray, depth, bands, count, R, S, acts, rgb_s[:M * 3].view(M, 3), dens[:M], ctx)
    work = None
    if ordered:
        work = torch.empty(ops.nerf_ordered_workspace(), dtype=torch.uint8, device='cuda')
        ops.nerf_ordered_attach(ctx, work)
    try:
        ops.nerf_bwd(flat, ray, depth, count, R, S, acts, rgb_s[:M * 3].view(M, 3), g_rgb, g_den, scr, grad[:flat.numel()],
                     gc[:R * 3].view(R, 3), gr[:R * 3].view(R, 3), ctx)
        torch.cuda.synchronize()
    finally:
        if ordered:
            ops.nerf_ordered_attach(ctx, None)
    for what, buf, n in (('rgb_samples', rgb_s, M * 3), ('density_samples', dens, M), ('g_center', gc, R * 3), ('g_ray', gr, R * 3),
                         ('params_grad', grad, flat.numel())):
        untouched(what, buf, n)
        assert bool(torch.isfinite(buf[:n]).all()), f'{what}: not finite, or a slot nobody wrote'
    return MR.make_run(flat, grad[:flat.numel()], acts, scr, rgb_s[:M * 3], dens[:M], g_rgb, g_den, gc[:R * 3].view(R, 3),
                       gr[:R * 3].view(R, 3), center, ray, depth, bands)


def check_stages(tag, stages, need=None, allow=None):
    """helpers.check at its default 8 ulps on every stage; allow: {stage: ulps} of the one documented exception (SINGLE_TERM_DY6)."""
    for name, got, (r64, r32, scale) in stages:
        assert bool(torch.isfinite(got).all()), f'{tag}: {name} is not finite'
        if need is not None and got.numel() <= 1 << 21:
            need[name] = max(need.get(name, 0.0), float(MR.ulps_needed(got, r64, r32, scale)))
            if need[name] > 8:
                print(f'ULPS-OVER {tag} {name}={need[name]:.2f}')
        check(f'{tag}: {name}', got, r64, r32, scale, **({'ulps': allow[name]} if allow and name in allow else {}))


def check_exact(tag, run, route):
    for what, ok in MR.exact_promises(run):
        assert ok, f'{tag}: {what}'
    for l, plane in enumerate(MR.mask_planes(run, rows_layout=route in ('fused', 'default'))):
        assert torch.equal(plane, run.A[f'a{l}'][:, :256] > 0), f'{tag}: mask plane {l} is not (own stored activation > 0)'


def report(tag, need):
    print(f'ULPS {tag} ' + ' '.join(f'{k}={v:.2f}' for k, v in need.items()))


# ------------------------------------------------------------------------------------------- every small and medium M, all routes
@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('i', range(len(C.SHAPES)), ids=[f'{R}x{S}' for R, S in C.SHAPES])
def test_every_stage_against_float64(i, route):
    (R, S), (progress, bd) = C.SHAPES[i], C.SETTINGS[i]
    tag = f'{route} {R}x{S} {progress} bd={bd}'
    run = run_pass(C.case(R, S, progress, bd), route)
    need = {}
    check_stages(tag, MR.all_stages(run), need)
    report(tag, need)
    check_exact(tag, run, route)
    raw = run.A['raw']
    if bd == 20.0:
        assert min(int((raw > 20).sum()), int((raw <= 20).sum())) >= C.MIN_PER_SIDE
    if bd == -30.0:
        assert bool((raw < -20).all())


@pytest.mark.parametrize('route', list(ROUTES))
@pytest.mark.parametrize('upstream', ['density_only', 'zero'])
def test_missing_upstream_gradients(upstream, route):
    """g_rgb = 0 with a random g_density: the colour head's gradients, dH, dHsum and dView are exactly zero, the operand maximum of
    dH is 0, and everything behind the density column still meets the rule.  Both zero: every gradient is exactly zero, and finite.

    The one exception to the 8 ulps, on the fused route with g_rgb = 0 only: DY6 is then the single product d raw * wd (its matrix
    part is exactly 0), so an entry is its own scale, and the fused chain stores a stage's output as the operand the next matrix
    instructions consume, (hi + lo) / s with s taking the TILE's largest magnitude to [2^14, 2^15): an absolute error of up to
    2^-25 / s, about 2^-40 of the tile maximum - the documented property of the three-product scheme, below the rounding of every sum
    the entry enters, but 44.33 ulps of an entry that is 1e-5 of its tile's maximum (5 of 497 408 entries).  DY6 there may take
    SINGLE_TERM_DY6 = 88 ulps, twice the measured need; the float32 reference needs 0.65."""
    R, S = C.MEDIUM
    tag = f'{route} {R}x{S} upstream {upstream}'
    run = run_pass(C.case(R, S, 'partly', 20.0, upstream), route)
    need = {}
    allow = {'DY6': SINGLE_TERM_DY6} if (upstream, route) == ('density_only', 'fused') else None
    check_stages(tag, MR.all_stages(run), need, allow)
    report(tag, need)
    check_exact(tag, run, route)
    for k in ('R0', 'br0', 'R1', 'br1') if upstream == 'density_only' else MR.PARAM_NAMES:
        assert bool((run.G[k] == 0).all()), f'{tag}: g.{k} is not exactly zero'
    for k in ('dH', 'dHsum', 'dView'):
        assert bool((run.X[k] == 0).all()), f'{tag}: {k} is not exactly zero'
    if upstream == 'zero':
        assert bool((run.g_center == 0).all()) and bool((run.g_ray == 0).all()), f'{tag}: ray gradients are not exactly zero'
        for k in ['d7', 'dEnc0', 'dEncS'] + [f'DY{l}' for l in range(7)]:
            assert bool((run.X[k] == 0).all()), f'{tag}: {k} is not exactly zero'
    else:
        assert float(run.G['W0'].abs().max()) > 0 and float(run.g_ray.abs().max()) > 0


# ---------------------------------------------------------------------------------------------- the two device-derived sizes
def tile_rows(M, cus):
    """Rows of the first two 64-row tiles, the last two, the first two of a fused work-group's second round (grid 2 cus) and the
    first 128-row tile of the second round of the 64-column GEMMs behind dEnc0 / dEncS (512 work-groups)."""
    tiles = (M + 63) // 64
    t = sorted({0, 1, 2 * cus, 2 * cus + 1, 1024, 1025, tiles - 2, tiles - 1})
    rows = torch.cat([torch.arange(64 * k, min(64 * k + 64, M)) for k in t if 0 <= k < tiles])
    return rows.cuda()


@pytest.mark.parametrize('which', ['second_tile', 'second_strip'])
def test_second_round_sizes_on_the_default_route(which):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R, S = C.second_tile_shape(cus) if which == 'second_tile' else C.second_strip_shape()
    M = R * S
    assert M > (2 * cus * 64 if which == 'second_tile' else 512 * 256) >= M - S
    tag = f'default {R}x{S}'
    run = run_pass(C.case(R, S, 'partly', 0.1), 'default')
    rows = tile_rows(M, cus)
    assert rows.numel() > 3 * 64 and int(rows.max()) == M - 1 and int((rows >= 2 * cus * 64).sum()) > 64
    need = {}
    check_stages(tag, MR.forward_stages(run, rows), need)
    check_stages(tag, MR.data_gradient_stages(run, rows), need)
    check_stages(tag, MR.ray_gradient_stages(run, torch.unique(rows // S)), need)
    # in full: the heads' stages, dHsum and every weight gradient
    check_stages(tag, MR.data_gradient_stages(run, names=('dH', 'd7[:,256]')), need)
    check_stages(tag, MR.head_sum_stages(run), need)
    check_stages(tag, MR.weight_gradient_stages(run), need)
    report(tag, need)
    check_exact(tag, run, 'default')


# ------------------------------------------------------------------------------------------------------------------ padding
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('route', list(ROUTES))
def test_padding_columns_reach_nothing(route):
    """W0 column 63, W4 column 319 and R0 columns 283 .. 287 set to 2^-7 (below each matrix's largest magnitude: no operand scale
    moves): the sample outputs, the ray gradients, every stored intermediate and every non-padding gradient are the bits of the run
    with zero padding, and the padding gradients stay exactly zero.  The weight-gradient products flush by float atomics in no fixed
    order, so their bits are compared where the flush is ordered: with the ordered-flush workspace on the split-precision routes;
    on the fp32 instructions at 4 x 16 = 64 rows, which one work-group adds to the zeroed block in one piece."""
    for (R, S), ordered, products in ((C.MEDIUM, route != 'fp32', route != 'fp32'), ((4, 16), False, True)):
        runs = [run_pass(C.case(R, S, 'open', 0.1, padding=p), route, ordered=ordered) for p in (0.0, 2.0 ** -7)]
        z, p = runs
        for name, cols in MR.PADDING.items():
            assert bool((p.P[name][:, list(cols)] == 2.0 ** -7).all()) and float(p.P[name].abs().max()) > 2.0 ** -7
            assert float(z.P[name].abs().max()) == float(p.P[name].abs().max())
        tag = f'{route} {R}x{S}'
        for k in ('rgb', 'density', 'g_center', 'g_ray'):
            assert torch.equal(_bits(getattr(z, k)), _bits(getattr(p, k))), f'{tag}: {k} depends on the padding columns'
        for k in ['enc', 'h', 'raw'] + [f'a{l}' for l in range(8)]:
            assert torch.equal(_bits(z.A[k]), _bits(p.A[k])), f'{tag}: {k} depends on the padding columns'
        for k, used in [('d7', 288), ('dH', 128), ('dEnc0', 63), ('dEncS', 63), ('dHsum', 128), ('dView', 27)] + [(f'DY{l}', 256) for l in range(7)]:
            # (column 63 of dEnc0 / dEncS and columns 27 .. 31 of dView are the products with the padding columns themselves: nobody reads them)
            assert torch.equal(_bits(z.X[k][:, :used]), _bits(p.X[k][:, :used])), f'{tag}: {k} depends on the padding columns'
        for what, ok in MR.exact_promises(p):
            assert ok, f'{tag}: {what}'
        for k in MR.PARAM_NAMES:
            if products or k in ('R1', 'br1', 'wd', 'bd'):
                assert torch.equal(_bits(z.G[k]), _bits(p.G[k])), f'{tag}: g.{k} depends on the padding columns'
        check_stages(tag + ' padded', MR.weight_gradient_stages(p))


# ------------------------------------------------------------------------------------------------------------- ordered flush
@pytest.mark.parametrize('route', ['fused', 'layered'])
def test_weight_gradients_with_the_ordered_flush(route):
    R, S = C.MEDIUM
    tag = f'{route} {R}x{S} ordered flush'
    run = run_pass(C.case(R, S, 'partly', 20.0), route, ordered=True)
    need = {}
    check_stages(tag, MR.weight_gradient_stages(run), need)
    check_stages(tag, MR.head_sum_stages(run), need)
    report(tag, need)
    check_exact(tag, run, route)
