"""Grounds tests/scene_ray_reference.py and tests/scene_ray_cases.py without a GPU:
  * the references are the project's functions: oracle.scene_nerf.composite / encode and bg_nerf.sample_depth_from_pdf, to float64
    rounding wherever those are defined;
  * the planted cases have the properties tests/test_hip_scene_ray_kernels.py rests on;
  * every error scale is sufficient: a float32 evaluation of the same operation in ANOTHER association (chunked scans, tree folds,
    a single-rounding multiply-add; plain numpy) passes the very rule the GPU test applies, at 8 ulps.  The largest ulps each output
    needs are printed (pytest -s) and recorded in the GPU test's docstring.  Only references pass through here, never a kernel."""
import numpy as np
import pytest
import torch

from oracle import scene_nerf as SN
from tests import scene_ray_cases as C
from tests import scene_ray_reference as RR
from tests.helpers import EPS, check, npf

F32 = np.float32
F64, F32T = torch.float64, torch.float32
FWD_KEYS = ('weights', 'rgb', 'depth', 'opacity', 'all_cumulated', 'depth_var', 'rgb_var')
BWD_KEYS = ('g_rgb_s', 'g_density', 'g_ray')


def close64(name, a, b, scale):
    a, b = npf(a), npf(b)
    assert a.shape == b.shape, name
    assert (np.abs(a - b) <= 1e-13 * (np.abs(b) + scale)).all(), name


# ------------------------------------------------------------------------------------------------------------------ compositing
@pytest.mark.parametrize('white', [False, True], ids=['black', 'white'])
@pytest.mark.parametrize('S', C.COMPOSITE_S)
def test_composite_reference_is_the_oracle_and_the_planted_rays_are_what_they_claim(S, white):
    c = C.composite_case(S)
    assert all(v.dtype == F32 for v in c.values()) and c['depth'].shape == (C.COMPOSITE_R, S)
    r64 = RR.composite(c, white, F64)
    for dt in RR.DTYPES:
        r = RR.composite(c, white, dt, grads=False)
        if S >= 2:
            o = SN.composite(*(RR.tt(c[k], dt) for k in ('rgb_s', 'density', 'depth', 'ray')), white_bg=white)
            for k in FWD_KEYS:
                assert r[k].dtype == dt
                close64(k, r[k], o[k], 1.0 if dt == F64 else 1e30)
                assert dt == F64 or np.array_equal(npf(r[k]), npf(o[k])), k
        assert all(bool(torch.isfinite(r[k]).all()) for k in FWD_KEYS)
    g32 = RR.composite(c, white, F32T)
    assert all(bool(torch.isfinite(g[k]).all()) for g in (r64, g32) for k in BWD_KEYS)
    w, T, op = npf(r64['weights']), npf(r64['T']), npf(r64['opacity'])
    lens = np.linalg.norm(c['ray'].astype(np.float64), axis=1)
    assert ((lens[[0, 10, 11, 12]] >= 0.7) & (lens[[0, 10, 11, 12]] <= 1.7)).all() and lens[4] < 2e-3 and lens[5] > 7e2
    assert (w[1, :-1] == 0).all() and w[1, -1] > 0.99                                  # all weight in the 1e10 interval
    k = min(3, S - 1)
    # behind the opaque sample T underflows in float32 (S = 512: intervals of 4e-3 leave 3e-17)
    assert (T[2, k + 1:] < (1e-15 if S == 512 else 1e-46)).all() and w[2, k] == T[2, k] > 0
    assert (w[3] == 0).all() and op[3] == 0 and (not white or (npf(r64['rgb'])[3] == 1).all())
    if S > 4:
        a = C.tie_start(S)
        assert (npf(r64['intv'])[6, a:a + 2] == 0).all() and (w[6, a:a + 2] == 0).all()
        assert S < 65 or (a + 2) // 64 > a // 64, 'the equal depths straddle a chunk boundary'
    assert 0 < npf(r64['sd'])[7, -1] < 0.02 and 0 < op[7] < 0.03                        # the last interval does not saturate
    assert op[8] == 1.0 or 1 - op[8] < 1e-12
    assert c['density'][9, -1] == 0 and w[9, -1] == 0 and (S == 1 or T[9, -1] > 0) and npf(r64['g_density'])[9, -1] != 0
    # dropping the g_weights term changes the gradients: the kernel's null branch is a different result
    no_gw = RR.composite(c, white, F64, with_gw=False)
    assert not np.array_equal(npf(no_gw['g_density']), npf(r64['g_density']))


def composite_table(S, white, with_gw):
    c = C.composite_case(S)
    r64, r32 = (RR.composite(c, white, dt, with_gw=with_gw) for dt in RR.DTYPES)
    m = RR.composite_chunked32(c, white, with_gw=with_gw)
    scales = dict(RR.composite_fwd_scales(c, r64, white), **RR.composite_bwd_scales(c, r64, white, with_gw))
    need = {}
    for k in FWD_KEYS + BWD_KEYS:
        if k == 'all_cumulated' and S < 2:
            continue
        sc = scales[k]
        need[k] = RR.ulps_needed(m[k], r64[k], r32[k], sc)
        check(f'{k} (chunked float32 numpy)', m[k], r64[k], r32[k], sc)
    return need


@pytest.mark.parametrize('with_gw', [True, False], ids=['gw', 'nogw'])
@pytest.mark.parametrize('white', [False, True], ids=['black', 'white'])
def test_composite_scales_let_a_chunked_float32_evaluation_through(white, with_gw):
    worst = {}
    for S in C.COMPOSITE_S:
        for k, v in composite_table(S, white, with_gw).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print(f'compositing, white_bg={white}, g_weights={with_gw}: ulps needed by the chunked float32 evaluation: '
          + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))
    assert max(worst.values()) <= 8


def test_composite_single_and_zero_length_ray():
    for S in C.COMPOSITE_S:
        c = C.composite_case(S, R=1)
        assert c['ray'].shape == (1, 3)
        zero = dict(c, ray=np.zeros((1, 3), F32))
        for dt in RR.DTYPES:
            r = RR.composite(zero, False, dt)
            assert (npf(r['weights']) == 0).all() and (npf(r['g_ray']) == 0).all() and bool(torch.isfinite(r['g_density']).all())
        assert (RR.composite_chunked32(zero, False)['g_ray'] == 0).all()


# ----------------------------------------------------------------------------------------------------------------- fine sampler
@pytest.mark.parametrize('N', C.PDF_N)
def test_pdf_cases_and_reference(N):
    w = C.pdf_weights(N)
    lo, hi = C.PDF_RANGE
    assert w.dtype == F32 and w.shape == (C.PDF_R, N) and (w >= 0).all()
    assert (w[1] > 0).sum() == 1 and (w[2] == 0).all() and np.allclose(w[5].sum(), 1) and 1e-7 < w[6].sum() < 4e-6
    assert N < 5 or ((w[3] == 0).mean() >= 0.75 and (w[3] > 0).any())
    assert (w[4] > 0).all() and (N == 1 or np.sort(w[4])[-2] <= 1.01e-7 * w[4].max())
    assert (w[7, :N // 2] == 0).all() and (w[8, N - N // 2:] == 0).all()
    inside, outside = C.pdf_depths(N, True), C.pdf_depths(N, False)
    assert inside.dtype == outside.dtype == F32 and (inside >= F32(lo)).all() and (inside <= F32(hi)).all()
    assert (N < 2 or (inside[:, 0] != np.sort(inside, 1)[:, 0]).any()) or N < 3                  # not handed over in order
    assert N < 3 or ((inside == F32(hi)).sum(1) >= 1).all() and all(len(np.unique(r)) < N for r in inside)
    nb = C.n_below(N)
    assert ((outside < F32(lo)).sum(1) == nb).all() and ((outside >= F32(hi)).sum(1) == N - nb).all()
    assert ((outside == F32(hi)).sum(1) == 1).all() and (N < 4 or all(len(np.unique(r)) < N for r in outside))
    for Nf in C.PDF_NF:
        for per_ray, det in C.PDF_GRIDS:
            grid = C.pdf_grid(Nf, per_ray, det)
            assert grid.dtype == F32 and grid.shape == ((C.PDF_R, Nf + 1) if per_ray else (Nf + 1,))
            u = RR.pdf_u(grid, C.PDF_R)
            assert (u >= 0).all() and (u < 1).all() and ((u > 0).all() if det else (u[:, 0] == 0).all() and (Nf < 4 or (np.diff(u, axis=1) < 0).any()))
            # the restated reference is the project's function given the project's bin edges: bit for bit in float32; in float64 up
            # to the float32 rounding of an edge difference, which the project's function forms before it promotes
            bins32 = torch.linspace(lo, hi, N + 1)
            for dt in RR.DTYPES:
                a, b = RR.pdf_fine(w, grid, C.PDF_RANGE, Nf, dt, bins=bins32), RR.pdf_project(w, grid, C.PDF_RANGE, Nf, dt)
                assert a.dtype == b.dtype == dt
                assert np.array_equal(npf(a), npf(b)) if dt == F32T else (np.abs(npf(a) - npf(b)) <= EPS * (hi - lo) / N).all()
            assert (npf(RR.pdf_project(w, grid, C.PDF_RANGE, Nf, F32T))[2] == F32(hi)).all()             # ray 2: all on dmax


def test_pdf_rules_let_float32_evaluations_through():
    """Rule (c) in cdf space on every ray, rule (d) on the smooth rays, for torch's float32 evaluation of the project's function and
    for the chunked numpy one."""
    worst = {}
    for N in C.PDF_N:
        w = C.pdf_weights(N)
        for Nf in C.PDF_NF:
            for per_ray, det in C.PDF_GRIDS:
                grid = C.pdf_grid(Nf, per_ray, det)
                u = RR.pdf_u(grid, C.PDF_R)
                p64, p32 = (RR.pdf_project(w, grid, C.PDF_RANGE, Nf, dt) for dt in RR.DTYPES)
                for name, x in (('torch', npf(p32)), ('chunked', RR.pdf_chunked32(w, grid, C.PDF_RANGE, Nf))):
                    assert np.isfinite(x).all() and (x[2] == F32(C.PDF_RANGE[1])).all()
                    for r in range(C.PDF_R):
                        need = RR.pdf_cdf_ulps(np.sort(x[r]), np.sort(u[r]), w[r], C.PDF_RANGE).max()
                        worst['cdf ' + name] = max(worst.get('cdf ' + name, 0.0), need)
                        assert need <= 8, (name, N, Nf, per_ray, det, r, need)
                    rows = list(C.SMOOTH_RAYS)
                    need = RR.ulps_needed(x[rows], p64[rows], p32[rows], C.PDF_RANGE[1])
                    worst['smooth ' + name] = max(worst.get('smooth ' + name, 0.0), need)
                    check(f'smooth rays ({name})', x[rows], p64[rows], p32[rows], C.PDF_RANGE[1])
    print('fine sampler: ulps needed: ' + ', '.join(f'{k} {v:.2f}' for k, v in worst.items()))


def test_pdf_cdf_rule_notices_a_shifted_sample():
    """The rule is not vacuous: a sample moved by a tenth of a bin of ordinary mass, or one pulled off dmax, fails it."""
    N, Nf = 64, 65
    w, grid = C.pdf_weights(N), C.pdf_grid(Nf, False, True)
    u = RR.pdf_u(grid, C.PDF_R)
    x = npf(RR.pdf_project(w, grid, C.PDF_RANGE, Nf, F32T))
    width = (C.PDF_RANGE[1] - C.PDF_RANGE[0]) / N
    moved = np.sort(x[5]) + 0.1 * width
    assert RR.pdf_cdf_ulps(moved, np.sort(u[5]), w[5], C.PDF_RANGE).max() > 1000
    assert RR.pdf_cdf_ulps(np.sort(x[2]) - 0.01, np.sort(u[2]), w[2], C.PDF_RANGE).max() > 1000


# --------------------------------------------------------------------------------------------------------------------- encoding
@pytest.mark.parametrize('progress', C.ENCODE_PROGRESS)
def test_encode_reference_scales_and_window(progress):
    w14 = RR.bands(progress)
    assert w14.dtype == F32T and w14.shape == (14,)
    open3, openv = int((w14[:10] > 0).sum()), int((w14[10:] > 0).sum())
    assert (open3, openv) == {0.45: (2, 1), 0.565: (6, 3), 1.0: (10, 4)}[progress]
    assert progress != 0.565 or float(w14[5]) == 0.5
    worst = [0.0, 0.0]
    for R, S in C.ENCODE_SHAPES:
        center, ray, depth = C.encode_case(R, S)
        assert (ray[0] != 0).sum() == 1 and abs(np.linalg.norm(ray[min(1, R - 1)].astype(np.float64)) - 1e-3) < 1e-9
        (p64, v64), (p32, v32) = (RR.encode(center, ray, depth, w14, dt) for dt in RR.DTYPES)
        # the oracle's own path: render() forms the points and mlp() the two encodings
        x = RR.tt(center, F64)[:, None] + RR.tt(ray, F64)[:, None] * RR.tt(depth, F64)[..., None]
        assert np.array_equal(npf(p64[..., :63]), npf(SN.encode(x, 10, w14[:10].double())))
        assert (npf(p64[..., 63]) == 0).all() and (npf(v64[:, 27:]) == 0).all()
        closed = np.concatenate([np.zeros(3, bool)] + [npf(w14[:10]) == 0] * 6 + [np.zeros(1, bool)])
        assert (npf(p32)[..., closed] == 0).all()
        s_p, s_v = RR.encode_scales(center, ray, depth, w14)
        assert s_p.shape == p64.shape and s_v.shape == v64.shape and (s_p[..., closed] == 0).all()
        mp, mv = RR.encode_fma32(center, ray, depth, w14)
        for i, (name, m, a, b, s) in enumerate((('points', mp, p64, p32, s_p), ('view', mv, v64, v32, s_v))):
            worst[i] = max(worst[i], RR.ulps_needed(m, a, b, s))
            check(f'{name} (single-rounding float32 numpy)', m, a, b, s)
    print(f'encoding, progress {progress}: ulps needed by the single-rounding float32 evaluation: points {worst[0]:.2f}, view {worst[1]:.2f}')


# -------------------------------------------------------------------------------------------------------------------- pose fold
@pytest.mark.parametrize('V', C.FOLD_V)
def test_fold_scale_lets_a_tree_fold_through(V):
    from tests.test_hip_scene_deterministic import fold_expression
    worst = 0.0
    for N in C.FOLD_N:
        a = C.fold_case(V, N)
        r64, r32 = (fold_expression(*(RR.tt(x, dt) for x in a)) for dt in RR.DTYPES)
        assert r64.shape == (V, 3, 4)
        m, s = RR.fold_tree32(*a), RR.fold_scale(*a)
        worst = max(worst, RR.ulps_needed(m, r64, r32, s))
        check('fold (strided sums and a tree, float32 numpy)', m, r64, r32, s)
    print(f'pose fold, V = {V}: ulps needed by the tree fold: {worst:.2f}')
