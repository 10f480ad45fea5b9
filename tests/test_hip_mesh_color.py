"""Vertex normals and colours on the GPU (poseprobe_amd.mesh.vertex_attributes, csrc/pp_mesh_color.hip) against the float64
restatement of their semantics (tests/mesh_color_reference.py, itself checked in tests/test_mesh_color_host.py): values, row
independence, what a call leaves alone, bounds, the export driver end to end, and the render path's own kernels chained by hand.

Tolerance of a comparison with the restatement: 4 x the largest difference between its float32 and its float64 run on the same
vertices, at least 4 ulps of 1.0 (colours and unit normals are of that magnitude).  The gradient of the DEFORMED sdf jumps across the
cell faces of the template at the warped point q: vertices whose q (float64) lies within 1e-3 voxel of a face are left out, at most
2 % of them; the plain template's gradient is continuous and nothing is left out there."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import mesh_color_reference as C
from tests.helpers import load

pytestmark = pytest.mark.gpu

ULP1 = float(np.finfo(np.float32).eps)
N_ITERS = 10000


@functools.lru_cache(maxsize=None)
def model():
    """The 24^3 drop-in model of the forward fixtures (warp net's last layer perturbed as the fixture stores it): this module's own."""
    from tests.test_hip_dropin import make_model
    return make_model(load('inference_g24.npz')).eval()


@functools.lru_cache(maxsize=None)
def params():
    return C.params(model())


@functools.lru_cache(maxsize=None)
def vertices(deform, resolution):
    """Model-coordinate vertices [Nv,3] float32 (numpy, read-only) of the deformed / plain zero level set at a lattice resolution."""
    from poseprobe_amd import mesh
    m = model()
    extract = mesh.voxurf_extract_deform_geometry if deform else mesh.voxurf_extract_geometry
    v, t = extract(m, m.xyz_min, m.xyz_max, resolution=resolution, threshold=0.0)
    v = np.ascontiguousarray(v, dtype=np.float32)
    assert len(v) > 257 and len(t) > 0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def restated(deform, resolution, progress):
    """(float64 run, float32 run, keep mask) of the restatement on vertices(deform, resolution) - computed once, shared."""
    v = vertices(deform, resolution)
    r64 = C.vertex_attributes(params(), v, use_deform=deform, progress=progress, dtype=torch.float64)
    r32 = C.vertex_attributes(params(), v, use_deform=deform, progress=progress, dtype=torch.float32)
    keep = ~C.face_mask(r64['q_u'], 1e-3) if deform else torch.ones(len(v), dtype=torch.bool)
    return r64, r32, keep


def attributes(v, deform, progress, **kw):
    """mesh.vertex_attributes with the model's stored progress set to `progress` (global_step=None reads it)."""
    from poseprobe_amd import mesh
    m = model()
    m.progress.data.fill_(progress)
    out = mesh.vertex_attributes(m, v, use_deform=deform, **kw)
    assert float(m.progress.detach()) == np.float32(progress)
    return out


def check_against_restatement(got, deform, resolution, progress, rows, name):
    r64, r32, keep = restated(deform, resolution, progress)
    keep = keep[rows]
    left_out = int((~keep).sum())
    assert left_out <= 0.02 * len(keep), f'{name}: {left_out} of {len(keep)} vertices lie within 1e-3 voxel of a cell face'
    for key in ('normals', 'colors'):
        a64, a32 = r64[key][rows][keep], r32[key][rows][keep].double()
        spread = float((a32 - a64).abs().max())
        tol = max(4 * spread, 4 * ULP1)
        err = float((got[key].cpu().double()[keep] - a64).abs().max())
        print(f'{name} {key}: {len(keep)} rows, {left_out} left out, float32/float64 spread {spread:.3e}, tolerance {tol:.3e}, '
              f'error {err:.3e}')
        assert err <= tol, f'{name} {key}: error {err:.3e} above {tol:.3e} (spread {spread:.3e})'


# ---- 1. against the float64 restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('progress', [0.5, 1.0])
@pytest.mark.parametrize('resolution', [20, 33])
@pytest.mark.parametrize('deform', [True, False])
def test_colours_and_normals_match_the_float64_restatement(deform, resolution, progress):
    v = vertices(deform, resolution)
    got = attributes(v, deform, progress)
    assert got['normals'].is_cuda and got['colors'].is_cuda
    assert got['normals'].dtype == got['colors'].dtype == torch.float32
    assert got['normals'].shape == got['colors'].shape == (len(v), 3)
    assert float(got['colors'].min()) >= 0 and float(got['colors'].max()) <= 1
    check_against_restatement(got, deform, resolution, progress, slice(None), f'deform={deform} resolution={resolution} progress={progress}')
    # an explicit global_step gives the weights of progress = global_step / N_iters, whatever the module stores
    from poseprobe_amd import mesh
    m = model()
    m.progress.data.fill_(0.25)
    again = mesh.vertex_attributes(m, torch.tensor(v, device='cuda'), use_deform=deform, global_step=int(progress * N_ITERS))
    assert float(m.progress.detach()) == 0.25
    assert torch.equal(again['colors'], got['colors']) and torch.equal(again['normals'], got['normals'])


@pytest.mark.parametrize('n,chunk', [(1, None), (63, None), (64, None), (65, None), (257, None), (257, 100)])
@pytest.mark.parametrize('deform', [True, False])
def test_row_counts_around_the_wavefront_and_the_work_group(deform, n, chunk):
    v = vertices(deform, 20)[:n]
    kw = {} if chunk is None else dict(chunk=chunk)
    got = attributes(v, deform, 0.5, **kw)
    assert got['colors'].shape == (n, 3)
    check_against_restatement(got, deform, 20, 0.5, slice(0, n), f'deform={deform} n={n} chunk={chunk}')


# ---- 2. independence and repeatability ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deform', [True, False])
def test_rows_are_independent_and_repeatable(deform):
    v = torch.tensor(vertices(deform, 20), device='cuda')
    Nv = len(v)
    a, b = attributes(v, deform, 0.5), attributes(v, deform, 0.5)
    assert a['colors'].data_ptr() != b['colors'].data_ptr()
    for key in ('normals', 'colors'):
        assert torch.equal(a[key], b[key]), key
    for chunk in (100, 256, Nv - 1, Nv, 4 * Nv):
        c = attributes(v, deform, 0.5, chunk=chunk)
        for key in ('normals', 'colors'):
            assert torch.equal(a[key], c[key]), (key, chunk)
    one = attributes(v[:70], deform, 0.5, chunk=1)
    for key in ('normals', 'colors'):
        assert torch.equal(a[key][:70], one[key]), key
    perm = torch.randperm(Nv, generator=torch.Generator().manual_seed(0)).cuda()
    p = attributes(v[perm], deform, 0.5, chunk=300)
    for key in ('normals', 'colors'):
        assert torch.equal(a[key][perm], p[key]), key


# ---- 3. nothing else moves ------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_the_model_alone():
    from poseprobe_amd import mesh
    m = model()
    m.progress.data.fill_(0.7)
    before = {k: t.detach().clone() for k, t in m.state_dict().items()}
    for deform in (True, False):
        mesh.vertex_attributes(m, vertices(True, 20), use_deform=deform)
        mesh.vertex_attributes(m, vertices(True, 20), use_deform=deform, global_step=3000)
    torch.cuda.synchronize()
    after = m.state_dict()
    assert set(after) == set(before)
    for k, t in before.items():
        assert torch.equal(after[k], t), k
    assert all(p.grad is None for p in m.parameters())


@functools.lru_cache(maxsize=None)
def engine():
    """A tiny object engine (the smoke test's) after one gradient pass: nonzero gradients, the buffers a view points into."""
    from oracle import voxurf_oracle as O
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    G, H, W, N, V = 16, 24, 24, 96, 3
    rs = syn.range_shape()
    views = syn.make_views(V, H, W)
    idx, jit = syn.step_randomness(V * H * W, N, seed=1)
    scene = O.Scene(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, output_range=float(rs.max()), rect_size=rs.tolist())
    P = O.init_params(scene, seed=2)
    eng = TrainEngine(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max())), V, H, W, N, device='cuda:0')
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    eng.zero_grads()
    eng.render_and_grads(torch.tensor(idx, dtype=torch.int32, device='cuda:0'), torch.tensor(jit, device='cuda:0'), 10)
    for t in (eng.flat.m, eng.k0_m):
        t.normal_()
    for t in (eng.flat.v, eng.k0_v):
        t.uniform_()
    torch.cuda.synchronize()
    return eng


def _engine_blocks(eng):
    return dict(flat_data=eng.flat.data, flat_grad=eng.flat.grad, flat_m=eng.flat.m, flat_v=eng.flat.v, k0_a=eng.k0[0], k0_b=eng.k0[1],
                k0_grad=eng.k0_grad, k0_m=eng.k0_m, k0_v=eng.k0_v, sdf=eng.sdf, se3=eng.se3, se3_grad=eng.se3_grad, se3_m=eng.se3_m,
                se3_v=eng.se3_v)


def test_a_call_through_the_engine_view_leaves_gradients_and_moments_alone(tmp_path):
    from poseprobe_amd import mesh
    from poseprobe_amd.trainer import DualBranchTrainer
    eng = engine()
    assert float(eng.flat.grad.abs().max()) > 0
    before = {k: t.detach().clone() for k, t in _engine_blocks(eng).items()}
    view = eng.voxurf_view()
    progress = float(view.progress.detach())
    g = torch.Generator().manual_seed(4)
    lo, hi = view.xyz_min.cpu(), view.xyz_max.cpu()
    pts = (lo + (hi - lo) * torch.rand(500, 3, generator=g)).cuda()
    for deform in (True, False):
        out = mesh.vertex_attributes(view, pts, use_deform=deform, global_step=8000, chunk=128)
        assert bool(torch.isfinite(out['colors']).all()) and bool(torch.isfinite(out['normals']).all())
    # the trainer's export: the same view, through the driver
    stub = types.SimpleNamespace(joint=types.SimpleNamespace(obj=eng))
    cfg = types.SimpleNamespace(basedir=str(tmp_path), expname='run')
    assert DualBranchTrainer.export_mesh(stub, cfg, resolution=20, extract_color=True, prefix='_t') == 0.0
    r = mesh.read_ply_attributes(os.path.join(str(tmp_path), 'run', 'meshes', 'deform_t.ply'))
    assert len(r['vertices']) > 0 and r['colors'] is not None and r['colors'].shape == r['vertices'].shape
    torch.cuda.synchronize()
    assert float(view.progress.detach()) == progress
    for k, t in _engine_blocks(eng).items():
        assert torch.equal(t, before[k]), k


# ---- 4. bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('deform', [True, False])
def test_rows_past_n_and_around_the_outputs_are_not_written(deform):
    from poseprobe_amd import mesh, ops
    from poseprobe_amd.grid import channels_last_view
    m = model()
    cfg = mesh._color_stage_config(m)
    n, cap, guard = 65, 128, 16
    f = dict(dtype=torch.float32, device='cuda')
    pts = torch.zeros(cap, 3, **f)
    pts[:n] = torch.tensor(vertices(deform, 20)[:n], device='cuda')
    flat = m._flat_params(pts.device)
    m.k0.ensure_layout()
    k0_cl, sdf = channels_last_view(m.k0.grid.detach()), m.sdf.grid.detach()[0, 0].contiguous()
    pe_w = torch.from_numpy(cfg.pe_weights(0.5)).cuda()
    warp_out = None
    if deform:
        warp_out = torch.empty(cap, 16, **f)
        count = torch.full((1,), n, dtype=torch.int32, device='cuda')
        acts = torch.empty(4, cap * 4, 128, **f)
        ops.warp_fwd(flat.view('warp'), pts, count, cap, cfg.out_range, acts, warp_out, getattr(m, 'pp_ctx', None))
    normal_all, feat_all = torch.full((guard + cap + guard, 3), 7.0, **f), torch.full((guard + cap + guard, ops.FEAT_LD), 7.0, **f)
    normal, feat = normal_all[guard:guard + cap], feat_all[guard:guard + cap]
    ops.vertex_feat(cfg.pp, sdf, flat.view('sdf_ab'), k0_cl, pts, warp_out, pe_w, 0, normal, feat)       # zero vertices: nothing happens
    torch.cuda.synchronize()
    assert bool((normal_all == 7.0).all()) and bool((feat_all == 7.0).all())
    ops.vertex_feat(cfg.pp, sdf, flat.view('sdf_ab'), k0_cl, pts, warp_out, pe_w, n, normal, feat)
    torch.cuda.synchronize()
    for whole, rows in ((normal_all, normal), (feat_all, feat)):
        assert bool((whole[:guard] == 7.0).all()) and bool((whole[guard + n:] == 7.0).all())
        assert bool(torch.isfinite(rows[:n]).all()) and not bool((rows[:n] == 7.0).all(dim=-1).any())
    assert bool((feat[:n, 57:] == 0).all())                                   # the zero padding the rgbnet's 64-column operand needs
    assert torch.equal(feat[:n, 54:57], normal[:n]) and torch.equal(feat[:n, 45:48], -normal[:n])
    with pytest.raises(RuntimeError, match='normal'):
        ops.vertex_feat(cfg.pp, sdf, flat.view('sdf_ab'), k0_cl, pts, warp_out, pe_w, n, normal[:n - 1], feat)
    got = mesh.vertex_attributes(m, np.zeros((0, 3), np.float32), use_deform=deform)
    assert got['normals'].shape == got['colors'].shape == (0, 3) and got['colors'].is_cuda


def test_other_colour_stage_shapes_are_refused():
    from poseprobe_amd import _lib, mesh, ops
    m = model()
    cfg = mesh._color_stage_config(m)
    sc = ops.make_scene(m.xyz_min.tolist(), m.xyz_max.tolist(), cfg.world_size, cfg.voxel_size, 1.0, 0., 1., 0., k0_dim=12, pos_pe=5,
                        view_pe=4)
    z = torch.zeros(24 * 24 * 24 * 12, device='cuda')
    with pytest.raises(_lib.PoseProbeError, match='shipped colour-stage shape'):
        ops.vertex_feat(sc, z, z, z, z, None, z, 4, z, z)


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------------
def test_validate_deform_mesh_writes_the_colours_of_vertex_attributes(tmp_path):
    from poseprobe_amd import dtu_eval, mesh
    m = model()
    m.progress.data.fill_(1.0)
    cfg = types.SimpleNamespace(basedir=str(tmp_path), expname='g24')
    v = vertices(True, 20)
    expect = np.floor(255 * np.clip(mesh.vertex_attributes(m, v)['colors'].cpu().numpy(), 0, 1)).astype(np.uint8)
    assert len(np.unique(expect)) > 1                                          # not one flat colour
    assert dtu_eval.validate_deform_mesh(m, cfg, resolution=20, extract_color=True, smooth=True) == 0.0
    r = mesh.read_ply_attributes(os.path.join(str(tmp_path), 'g24', 'meshes', 'deform.ply'))
    assert np.array_equal(r['vertices'], v) and r['colors'].dtype == np.uint8 and np.array_equal(r['colors'], expect)
    assert r['normals'] is None and len(r['triangles']) > 0
    scale = np.diag([3.0, 3.0, 3.0, 1.0])
    scale[:3, 3] = [1.0, -2.0, 0.5]
    dtu_eval.validate_deform_mesh(m, cfg, resolution=20, extract_color=True, world_space=True, scale_mats_np=scale, prefix='_w')
    w = mesh.read_ply_attributes(os.path.join(str(tmp_path), 'g24', 'meshes', 'deform_w.ply'))
    assert np.array_equal(w['vertices'], (v * scale[0, 0] + scale[:3, 3][None]).astype(np.float32))
    assert np.array_equal(w['colors'], expect) and np.array_equal(w['triangles'], r['triangles'])
    without = dtu_eval.validate_deform_mesh(m, cfg, resolution=20, prefix='_grey')
    assert without == 0.0 and mesh.read_ply_attributes(os.path.join(str(tmp_path), 'g24', 'meshes', 'deform_grey.ply'))['colors'] is None


# ---- 6. the render path's kernels chained by hand ----------------------------------------------------------------------------------
def test_agrees_with_the_render_path_chained_by_hand():
    """pp_geometry_fwd, then -g / (|g| + 1e-5) in torch, then pp_color_feat_fwd with ray_id = arange, then pp_rgbnet_fwd: the same
    device code fed through tables.  The one difference is |g|: torch's norm against the kernel's fma chain, each within an ulp of
    the exact value, so the view direction and the normal differ by up to 2 ulps per component.  Bound for the normals: 4 ulps of
    1.0.  For the colours: the 12 columns that carry them (view, its sine and cosine, normal) move by at most 2 ulps each, the
    rgbnet is Lipschitz with the product of its layers' spectral norms (ReLU is 1-Lipschitz, the sigmoid 1/4), plus 4 ulps for the
    kernel's own rounding of different inputs.  The float64 test above is the yardstick, not this one."""
    from poseprobe_amd import mesh, ops
    from poseprobe_amd.grid import channels_last_view
    m = model()
    cfg = mesh._color_stage_config(m)
    v = torch.tensor(vertices(True, 20), device='cuda')
    n = len(v)
    got = attributes(v, True, 0.5)
    f = dict(dtype=torch.float32, device='cuda')
    flat = m._flat_params(v.device)
    ctx = getattr(m, 'pp_ctx', None)
    m.k0.ensure_layout()
    k0_cl, sdf = channels_last_view(m.k0.grid.detach()), m.sdf.grid.detach()[0, 0].contiguous()
    pe_w = torch.from_numpy(cfg.pe_weights(0.5)).cuda()
    count = torch.full((1,), n, dtype=torch.int32, device='cuda')
    ray_id = torch.arange(n, dtype=torch.int32, device='cuda')
    warp_out, acts = torch.empty(n, 16, **f), torch.empty(4, n * 4, 128, **f)
    alpha, gradient, feat = torch.empty(n, **f), torch.empty(n, 3, **f), torch.empty(n, ops.FEAT_LD, **f)
    rgb, rgb_acts = torch.empty(n, 3, **f), torch.empty(3, n, 128, **f)
    ops.warp_fwd(flat.view('warp'), v, count, n, cfg.out_range, acts, warp_out, ctx)
    ops.geometry_fwd(cfg.pp, sdf, flat.view('sdf_ab'), v, warp_out, torch.zeros(n, 3, **f), ray_id, count, n, 1.0, alpha, gradient,
                     None, None, None)
    view = (-gradient / (gradient.norm(2, -1, keepdim=True) + 1e-5)).contiguous()
    ops.color_feat_fwd(cfg.pp, k0_cl, v, view, ray_id, gradient, pe_w, count, n, feat)
    ops.rgbnet_fwd(flat.view('rgbnet'), feat, count, n, rgb_acts, rgb, ctx)
    d_normal = float((got['normals'] - feat[:, 54:57]).abs().max())
    d_color = float((got['colors'] - rgb).abs().max())
    layers = [W.double() for W, _ in params()['rgbnet']]
    lipschitz = 0.25 * float(torch.linalg.matrix_norm(layers[0][:, 45:57], ord=2))
    for W in layers[1:]:
        lipschitz *= float(torch.linalg.matrix_norm(W, ord=2))
    bound_color = lipschitz * np.sqrt(12.0) * 2 * ULP1 + 4 * ULP1
    print(f'hand-chained render path: largest difference normals {d_normal:.3e} (bound {4 * ULP1:.3e}), colours {d_color:.3e} '
          f'(bound {bound_color:.3e}, Lipschitz {lipschitz:.3f})')
    assert d_normal <= 4 * ULP1 and d_color <= bound_color
