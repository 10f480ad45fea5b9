"""The scene branch's ray kernels (csrc/pp_nerf.hip) one at a time against float64, on the seeded inputs of tests/scene_ray_cases.py
with the edge cases planted: pp_nerf_composite_fwd / _bwd, pp_nerf_sample_pdf, k_nerf_encode (through pp_nerf_fwd's activation
block) and pp_nerf_c2w_fold.  References and error scales: tests/scene_ray_reference.py, pinned on the CPU by
tests/test_scene_ray_reference.py.

Assertions, and no other tolerance:
  * helpers.check:  |hip - ref64| <= 2 |ref32 - ref64| + 8 eps32 * scale.  The kernel gets the very float32 inputs of both references;
    the scale is the sum of the magnitudes of the terms behind an entry (scene_ray_reference.*_scales say which);
  * the fine sampler's values in cdf space (scene_ray_reference.pdf_cdf_ulps, 8 ulps as well): dx / du = width / mass makes positions
    ill-conditioned where a bin holds 1e-7 of the mass;
  * exact promises with np.array_equal / ==;
  * every output buffer carries guard rows holding a sentinel that must come back unchanged, and is prefilled (sentinel or NaN) so
    that a slot nobody wrote shows.

A property of k_nerf_composite_bwd that the scale of g_density states: the kernel forms the sum behind sample j as "chunk total -
inclusive prefix" of its 64-sample chunk, so the prefix of j's own chunk is a term of the sum behind the entry - the scale counts
every sample from the START of j's chunk to the end of the ray, not only those behind j.  For the last sample that difference is
exactly zero (the kernel reads the chunk total at the last valid lane) and the scale counts nothing: the 1e10-long interval would
multiply any residue.  This is a fact about the algorithm, not a licence for other errors.

ulps that a float32 evaluation in ANOTHER association needs under these rules on these inputs (CPU, plain numpy: 64-wide chunked
scans with a carry, strided sums folded by a tree, a single-rounding multiply-add; tests/test_scene_ray_reference.py prints them),
against the 8 allowed:
    compositing   weights 0.67  rgb 0.62  depth 0.39  opacity 0.37  all_cumulated 0.41  depth_var 0.34  rgb_var 0.37
                  g_rgb_samples 1.57  g_density 0.62  g_ray 0.67
    fine sampler  cdf space 3.17 (torch's float32: 0.93)   positions on the smooth rays 5.17
    encoding      points 0.85  view 0.56
    pose fold     0.21
and what the kernels themselves needed on an MI355X when these tests were written (a record, not a bound: the bound stays 8):
    compositing   weights 0.50  rgb 0.65  depth 0.31  opacity 0.27  all_cumulated 0.20  depth_var 0.01  rgb_var 0.10
                  g_rgb_samples 1.57  g_density 0.91 (0.56 without g_weights)  g_ray 0.62 (0.52)
    fine sampler  cdf space 1.00   positions on the smooth rays 1.76
    encoding      points 0.32  view 0.21
    pose fold     0.21

One-line mutations of the kernels that these tests were tried against, each caught: the forward carry read at lane 62 (rgb, weights at
S >= 65), carry_arr[c - 1] in the backward (g_density at S >= 65; at S = 65 only ray 9 sees it, whose last density is 0), go without
its white_bg term (g_density on white), `cdf[mid] < u` in the sampler (the all-zero ray with u = 0: dmin instead of dmax),
`n < N - 1` in the fold (every N), sines for cosines in nerf_enc_elem (the encoding's values).
"""
import numpy as np
import pytest
import torch

from tests import scene_ray_cases as C
from tests import scene_ray_reference as RR
from tests.helpers import check, cu
from tests.test_hip_ray_kernels import GUARD, SENT, full, host, untouched
from tests.test_hip_scene import OUT_LD
from tests.test_hip_scene_deterministic import fold_expression

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float('nan')


# ------------------------------------------------------------------------------------------------------------------ compositing
def run_composite(c, white):
    """Forward, backward with g_weights and backward without, each against its float64 reference; -> the numpy outputs."""
    from poseprobe_amd import ops
    R, S = c['depth'].shape
    dev = {k: cu(v) for k, v in c.items()}
    rgb_s, dens = dev['rgb_s'].reshape(R * S, 3), dev['density'].reshape(R * S)
    fwd = dict(rgb=full(R + GUARD, 3), depth=full(R + GUARD), opacity=full(R + GUARD), weights=full(R + GUARD, S),
               all_cumulated=full(R + GUARD), rgb_var=full(R + GUARD), depth_var=full(R + GUARD))
    ops.nerf_composite_fwd(rgb_s, dens, dev['depth'], dev['ray'], R, S, white, fwd['rgb'], fwd['depth'], fwd['opacity'],
                           fwd['weights'], fwd['all_cumulated'], fwd['rgb_var'], fwd['depth_var'])
    r64, r32 = (RR.composite(c, white, dt) for dt in RR.DTYPES)
    scales = RR.composite_fwd_scales(c, r64, white)
    out = {}
    for k, buf in fwd.items():
        untouched(k, buf, R)
        out[k] = host(buf)[:R]
        assert np.isfinite(out[k]).all(), k
        if k == 'all_cumulated' and S < 2:            # the oracle indexes T[:, -2]; the kernel returns 1 for a single sample
            assert (out[k] == 1).all()
            continue
        check(k, out[k], r64[k], r32[k], scales[k])
    # backward on the kernel's OWN forward weights, as bg_nerf._Composite runs it
    w_own = fwd['weights'][:R]
    for with_gw, (b64, b32) in ((True, (r64, r32)), (False, [RR.composite(c, white, dt, with_gw=False) for dt in RR.DTYPES])):
        g_rgb_s, g_dens, g_ray = full((R + GUARD) * S, 3), full((R + GUARD) * S), full(R + GUARD, 3)
        ops.nerf_composite_bwd(rgb_s, dens, dev['depth'], dev['ray'], w_own, R, S, white, dev['g_rgb'], dev['g_depth'],
                               dev['g_opacity'], dev['g_weights'] if with_gw else None, g_rgb_s, g_dens, g_ray)
        bs = RR.composite_bwd_scales(c, r64, white, with_gw)
        tag = '' if with_gw else ' (g_weights = None)'
        for k, buf, rows, shape in (('g_rgb_s', g_rgb_s, R * S, (R, S, 3)), ('g_density', g_dens, R * S, (R, S)), ('g_ray', g_ray, R, (R, 3))):
            untouched(k + tag, buf, rows)
            got = host(buf)[:rows].reshape(shape)
            assert np.isfinite(got).all(), k + tag
            check(k + tag, got, b64[k], b32[k], bs[k])
            out[k + tag] = got
    return out


@pytest.mark.parametrize('white', [False, True], ids=['black', 'white'])
@pytest.mark.parametrize('S', C.COMPOSITE_S)
def test_composite_fwd_bwd_on_planted_rays(S, white):
    """13 rays (the last work-group holds one) with the planted rays of scene_ray_cases.composite_case; S from one sample to the
    eight chunks of carry_arr[8]."""
    c = C.composite_case(S)
    out = run_composite(c, white)
    assert (out['weights'][3] == 0).all() and out['opacity'][3] == 0, 'zero density: weights and opacity are exactly 0'
    if white:
        assert (out['rgb'][3] == 1).all(), 'zero density on white: rgb is exactly 1'


@pytest.mark.parametrize('S', C.COMPOSITE_S)
def test_composite_single_ray_and_zero_length_ray(S):
    c = C.composite_case(S, R=1)
    run_composite(c, False)
    run_composite(c, True)
    zero = dict(c, ray=np.zeros((1, 3), F32))
    for white in (False, True):
        out = run_composite(zero, white)
        assert (out['g_ray'] == 0).all() and (out['g_ray (g_weights = None)'] == 0).all(), 'a ray of length 0 has g_ray = 0'
        assert (out['weights'] == 0).all()


# ----------------------------------------------------------------------------------------------------------------- fine sampler
def run_pdf(w, depth, grid, Nf):
    from poseprobe_amd import ops
    R, N = w.shape
    out = full(R + GUARD, N + Nf)
    out[:R] = NAN
    ops.nerf_sample_pdf(cu(w), cu(depth), cu(grid), Nf, C.PDF_RANGE, out[:R])
    untouched('depth_out', out, R)
    got = host(out)[:R]
    assert np.isfinite(got).all(), 'a slot was not written (two values shared a rank) or a sample is not finite'
    assert (got[:, 1:] >= got[:, :-1]).all(), 'not ascending'
    return got


@pytest.mark.parametrize('Nf', C.PDF_NF)
@pytest.mark.parametrize('N', C.PDF_N)
def test_sample_pdf_structure_and_values(N, Nf):
    """Shared / per-ray and deterministic / random grids.  With every coarse depth outside the range the Nf fine samples sit in a
    known slice, sorted, and pair with the sorted u (x is monotone in u); with the coarse depths inside, the output is the sorted
    union of those fine samples and the coarse depths, bit for bit."""
    w = C.pdf_weights(N)
    inside, outside = C.pdf_depths(N, True), C.pdf_depths(N, False)
    nb, dmax = C.n_below(N), F32(C.PDF_RANGE[1])
    rows = list(C.SMOOTH_RAYS)
    for per_ray, det in C.PDF_GRIDS:
        tag = f'per_ray={per_ray} det={det}'
        grid = C.pdf_grid(Nf, per_ray, det)
        got = run_pdf(w, outside, grid, Nf)
        fine = got[:, nb:nb + Nf]
        # (a) structure
        assert np.array_equal(np.delete(got, np.s_[nb:nb + Nf], axis=1), np.sort(outside, 1)), f'{tag}: coarse depths changed'
        assert np.array_equal(run_pdf(w, inside, grid, Nf), np.sort(np.concatenate([inside, fine], 1), 1)), f'{tag}: merge'
        # (b) nothing to sample from: every sample on dmax
        assert (fine[2] == dmax).all(), f'{tag}: the all-zero ray'
        # (c) values in cdf space
        u = np.sort(RR.pdf_u(grid, C.PDF_R), 1)
        for r in range(C.PDF_R):
            need = RR.pdf_cdf_ulps(fine[r], u[r], w[r], C.PDF_RANGE)
            assert need.max() <= 8, f'{tag} ray {r}: sample {need.argmax()} needs {need.max():.3g} ulps in cdf space (x {fine[r, need.argmax()]!r})'
        # (d) positions on the smooth rays
        p64, p32 = (np.sort(RR.pdf_project(w, grid, C.PDF_RANGE, Nf, dt).numpy()[rows], 1) for dt in RR.DTYPES)
        check(f'{tag}: smooth rays', fine[rows], p64, p32, float(dmax))


@pytest.mark.parametrize('N,Nf', [(257, 64), (64, 257)])
def test_sample_pdf_refuses_sizes_beyond_256(N, Nf):
    from poseprobe_amd import ops
    from poseprobe_amd._lib import PoseProbeError
    out = full(2 + GUARD, N + Nf)
    with pytest.raises(PoseProbeError, match='bad sizes'):
        ops.nerf_sample_pdf(cu(np.ones((2, N), F32)), cu(np.ones((2, N), F32)), cu(np.linspace(0, 1, Nf + 1, dtype=F32)), Nf,
                            C.PDF_RANGE, out[:2])
    torch.cuda.synchronize()
    untouched('depth_out', out, 0)


# --------------------------------------------------------------------------------------------------------------------- encoding
@pytest.fixture(scope='module')
def net():
    from poseprobe_amd import bg_nerf
    return bg_nerf.NeRF(bg_nerf.default_options(barf_c2f=C.BARF_C2F), device='cuda')


@pytest.mark.parametrize('progress', C.ENCODE_PROGRESS)
@pytest.mark.parametrize('R,S', C.ENCODE_SHAPES)
def test_encoding_in_the_activation_block(net, R, S, progress):
    """After one pp_nerf_fwd: the [M, 64] encoding at the front of the activation block, its skip copy in columns 256 .. 319 of layer
    3's output rows and the view encoding in columns 256 .. 287 of layer 7's, against oracle.scene_nerf.encode with the window
    weights the kernel was handed.  A wavefront takes four consecutive samples: where M = R S is no multiple of 4 the ray changes
    inside them and the last wavefront returns early."""
    from poseprobe_amd import ops
    center, ray, depth = C.encode_case(R, S)
    w14 = RR.bands(progress)
    M = R * S
    n_acts, _ = ops.nerf_workspace(M, R)
    acts = torch.full((n_acts + GUARD,), NAN, device='cuda')
    acts[n_acts:] = SENT
    rgb_s, dens = full(M + GUARD, 3), full(M + GUARD)
    count = torch.tensor([M], dtype=torch.int32, device='cuda')
    ops.nerf_fwd(net.flat, cu(center), cu(ray), cu(depth), cu(w14), count, R, S, acts, rgb_s, dens, net.ctx)
    untouched('acts', acts, n_acts)
    untouched('rgb_samples', rgb_s, M)
    untouched('density_samples', dens, M)
    assert bool(torch.isfinite(rgb_s[:M]).all()) and bool(torch.isfinite(dens[:M]).all())
    off = [M * 64]
    for ld in OUT_LD:
        off.append(off[-1] + M * ld)
    enc = host(acts[:M * 64].view(M, 64)).reshape(R, S, 64)
    skip = host(acts[off[3]:off[4]].view(M, OUT_LD[3])[:, 256:]).reshape(R, S, 64)
    view = host(acts[off[7]:off[8]].view(M, OUT_LD[7])[:, 256:]).reshape(R, S, 32)
    (p64, v64), (p32, v32) = (RR.encode(center, ray, depth, w14, dt) for dt in RR.DTYPES)
    s_p, s_v = RR.encode_scales(center, ray, depth, w14)
    check('encoding', enc, p64, p32, s_p)
    check('view encoding', view[:, 0], v64, v32, s_v)
    assert np.array_equal(skip, enc), 'the skip copy is the encoding bit for bit'
    assert np.array_equal(view, np.broadcast_to(view[:, :1], view.shape)), 'one view encoding per ray, bit for bit'
    assert (enc[..., 63] == 0).all() and (view[..., 27:] == 0).all(), 'padding columns'
    closed3, closedv = w14[:10].numpy() == 0, w14[10:].numpy() == 0
    assert closed3.sum() == {0.45: 8, 0.565: 4, 1.0: 0}[progress]
    assert (enc[..., 3:63].reshape(R, S, 3, 2, 10)[..., closed3] == 0).all(), 'a band whose window weight is 0 gives exactly 0'
    assert (view[..., 3:27].reshape(R, S, 3, 2, 4)[..., closedv] == 0).all()


# -------------------------------------------------------------------------------------------------------------------- pose fold
@pytest.mark.parametrize('V', C.FOLD_V)
@pytest.mark.parametrize('N', C.FOLD_N)
def test_c2w_fold_tail_and_idle_views(N, V):
    from poseprobe_amd import ops
    a = C.fold_case(V, N)
    r64, r32 = (fold_expression(*(RR.tt(x, dt) for x in a)) for dt in RR.DTYPES)
    dev = [cu(x) for x in a]
    outs = []
    for _ in range(2):
        out = full(C.FOLD_ROWS + GUARD, 3, 4)
        ops.nerf_c2w_fold(*dev, out[:C.FOLD_ROWS])
        untouched('g_c2w', out, C.FOLD_ROWS)
        outs.append(host(out)[:C.FOLD_ROWS])
    check('g_c2w', outs[0][:V], r64, r32, RR.fold_scale(*a))
    assert (outs[0][V:] == 0).all(), 'views that are not in play'
    assert np.array_equal(outs[0], outs[1]), 'two calls differ'
