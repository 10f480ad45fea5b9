"""Host side of the coloured mesh export (no GPU): the float64-capable restatement of the vertex attributes
(tests/mesh_color_reference.py) checked against mathematics, the PLY attributes, the export driver with the mesh functions
replaced, and the declaration of the new entry point."""
import functools
import hashlib
import math
import os
import types

import numpy as np
import pytest
import torch

from tests import mesh_color_reference as C
from tests.helpers import load


# ---- the restatement itself ------------------------------------------------------------------------------------------------------
G, BOX, RADIUS = 48, 1.0, 0.7


@functools.lru_cache(maxsize=None)
def sphere_params(zero_warp=True):
    """A template of its own: the signed distance to a sphere of radius 0.7 on a 48^3 grid over [-1, 1]^3, random colour grid and
    nets; the warp net's last layer zero (the reference's initialisation) or small."""
    g = torch.Generator().manual_seed(3)
    ax = torch.linspace(-BOX, BOX, G, dtype=torch.float64)
    sdf = (torch.stack(torch.meshgrid(ax, ax, ax, indexing='ij'), -1).norm(dim=-1) - RADIUS).float()
    lin = lambda o, i, s=1.0: (torch.randn(o, i, generator=g) * s / math.sqrt(i), torch.randn(o, generator=g) * 0.1)
    warp = [lin(128, 3), lin(128, 128), lin(128, 128), lin(128, 128), lin(4, 128, 0.02)]
    if zero_warp:
        warp[4] = (torch.zeros(4, 128), torch.zeros(4))
    return dict(xyz_min=torch.full((3,), -BOX), xyz_max=torch.full((3,), BOX), sdf=sdf, k0=torch.randn(12, G, G, G, generator=g) * 0.3,
                sdf_alpha=torch.tensor([10.0]), sdf_beta=torch.tensor([2.0]),
                rgbnet=[lin(128, 57), lin(128, 128), lin(128, 128), lin(3, 128)], warp=warp, out_range=0.8,
                voxel_size=float(((2 * BOX) ** 3 / G ** 3) ** (1 / 3)), barf_c2f=(0.6, 1.0), N_iters=10000, progress=1.0)


def shell_points(n, seed, band):
    """n points with | |p| - RADIUS | < band: where the vertices of the sphere's mesh lie."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(n, 3, generator=g, dtype=torch.float64)
    rho = RADIUS + (torch.rand(n, 1, generator=g, dtype=torch.float64) * 2 - 1) * band
    return d / d.norm(dim=-1, keepdim=True) * rho


def test_zeroed_last_colour_layer_gives_the_sigmoid_of_its_bias():
    P = dict(sphere_params(False))
    bias = torch.tensor([-1.5, 0.25, 2.0])
    P['rgbnet'] = P['rgbnet'][:3] + [(torch.zeros(3, 128), bias)]
    pts = shell_points(64, 0, 0.3)
    for deform in (True, False):
        for dtype in (torch.float32, torch.float64):
            r = C.vertex_attributes(P, pts, use_deform=deform, progress=0.8, dtype=dtype)
            assert r['colors'].dtype == dtype and r['colors'].shape == (64, 3)
            assert torch.equal(r['colors'], torch.sigmoid(bias.to(dtype)).expand(64, 3))


def test_deformed_and_plain_gradients_agree_without_a_deformation():
    """Warp's last layer zero: q = p and sdf = mapped template(p).  g is then the gradient of the trilinear interpolant, the plain
    g the interpolated central differences: two estimates of grad F, F = A (sigmoid(B (|p| - r)) - 0.5).  Every component of either is a
    convex combination of difference quotients of F along axis a over segments between nodes of the cell of p and their axis
    neighbours, i.e. of d_a F at points within (sqrt(3) + 1) h of p (mean value theorem; h = node spacing) - times one positive
    factor per estimate (1 / h against 1 / voxel_size: the reference's two unit conventions), which the normal does not see.  With
    K >= the Hessian norm of F there and m <= |grad F(p)|, each estimate is within delta = sqrt(3) K (sqrt(3) + 1) h of grad F(p), each
    normal within asin(delta / m) of the true one, and the two normals within twice that angle of each other."""
    P = sphere_params(True)
    h = 2 * BOX / (G - 1)
    band = h
    pts = shell_points(4000, 1, band)
    d = C.vertex_attributes(P, pts, use_deform=True, dtype=torch.float64)
    p = C.vertex_attributes(P, pts, use_deform=False, dtype=torch.float64)
    away = ~C.face_mask(d['q_u'], 1e-3)
    assert away.float().mean() > 0.98
    # F = phi(rho): Hessian eigenvalues phi'' (radial) and phi' / rho (tangential, twice)
    A, B = 10.0, 2.0                                                # softplus(., beta=10) of 10 and of 2 to 2e-9
    reach = band + (math.sqrt(3) + 1) * h
    s = torch.linspace(-reach, reach, 20001, dtype=torch.float64)
    sg = torch.sigmoid(B * s)
    d1, d2 = A * B * sg * (1 - sg), A * B * B * sg * (1 - sg) * (1 - 2 * sg)
    K = max(float(d2.abs().max()), float((d1 / (RADIUS + s)).max()))
    m = float((A * B * torch.sigmoid(torch.tensor(B * band)) * (1 - torch.sigmoid(torch.tensor(B * band)))))
    delta = math.sqrt(3) * K * (math.sqrt(3) + 1) * h
    bound = 2 * math.asin(delta / m)
    angle = torch.acos((d['normals'] * p['normals']).sum(-1).clamp(-1, 1))[away]
    print(f'largest angle between the two normals {float(angle.max()):.4f} rad, bound {bound:.4f} rad (delta {delta:.3f}, m {m:.3f})')
    assert delta < m and bound < 1.0                               # the bound says something: a swapped axis or sign is ~ pi / 2 or more
    assert float(angle.max()) <= bound
    # the factor between the two estimates is the reference's: node spacing against voxel_size
    ratio = (p['gradient'].norm(dim=-1) / d['gradient'].norm(dim=-1))[away]
    assert abs(float(ratio.median()) - h / P['voxel_size']) < 0.02


@pytest.mark.parametrize('zero_warp', [True, False])
def test_normals_of_a_sphere_point_outward(zero_warp):
    P = sphere_params(zero_warp)
    pts = shell_points(2000, 2, 2 * BOX / (G - 1))
    for deform in (True, False):
        r = C.vertex_attributes(P, pts, use_deform=deform, dtype=torch.float64)
        out = (r['normals'] * pts).sum(-1)
        assert float(out.min()) > 0, (deform, float(out.min()))
        nn = r['normals'].norm(dim=-1)
        assert float(nn.max()) <= 1 and float(nn.min()) > 1 - 1e-5          # g / (|g| + 1e-5), |g| of a few units
        assert torch.equal(r['feat'][:, 54:57], r['normals']) and torch.equal(r['feat'][:, 45:48], -r['normals'])
        assert float(r['colors'].min()) >= 0 and float(r['colors'].max()) <= 1


def test_band_weights_follow_progress():
    """Closed bands switch the encodings off: rows at progress 0.6 (the start of the window) carry zeros there, the raw coordinates
    and the normal stay."""
    P = sphere_params(False)
    pts = shell_points(16, 4, 0.1)
    r = C.vertex_attributes(P, pts, progress=0.6, dtype=torch.float64)
    f = r['feat']
    assert float(f[:, 15:45].abs().max()) == 0 and float(f[:, 48:54].abs().max()) == 0
    assert torch.equal(f[:, 12:15], (pts + BOX) / (2 * BOX))
    full = C.vertex_attributes(P, pts, progress=1.0, dtype=torch.float64)['feat']
    assert float(full[:, 15:45].abs().max()) > 0.5 and float(full[:, 48:54].abs().max()) > 0.5


def test_fixture_vertices_stay_within_the_exclusion_budget():
    """The GPU test (tests/test_hip_mesh_color.py) leaves out vertices whose warped point lies within 1e-3 voxel of a cell face, at most
    2 % of them: the fixture's own perturbation of the warp net's last layer stays far inside that on both lattices."""
    P = C.params(load('inference_g24.npz'))
    for res in (20, 33):
        v = C.deform_vertices(P, res)
        r = C.vertex_attributes(P, v, use_deform=True, progress=0.5, dtype=torch.float64)
        frac = float(C.face_mask(r['q_u'], 1e-3).float().mean())
        print(f'resolution {res}: {len(v)} vertices, {frac:.4%} within 1e-3 voxel of a face')
        assert len(v) > 257 and frac <= 0.01


# ---- PLY attributes --------------------------------------------------------------------------------------------------------------
def _mesh(seed=5):
    rs = np.random.RandomState(seed)
    return rs.randn(7, 3).astype(np.float32), rs.randint(0, 7, (4, 3)).astype(np.int32), rs.rand(7, 3)


def test_write_ply_without_the_new_keyword_writes_the_bytes_it_wrote(tmp_path):
    """Digests of the files the function wrote for this mesh before it knew `vertex_normals`."""
    from poseprobe_amd import mesh
    v, t, c = _mesh()
    recorded = {'plain': (305, 'f8577dfb0ccd957bfb088ccd0643bd82f8dcb9e7be513d82168d370876a1fd12'),
                'colors': (386, 'd420d9c366104a9c097e142494ffcab7f7bfdbfafeed69c01a03b80bed526932')}
    for name, kw in (('plain', {}), ('colors', dict(vertex_colors=c))):
        path = str(tmp_path / f'{name}.ply')
        mesh.write_ply(path, v, t, **kw)
        data = open(path, 'rb').read()
        assert (len(data), hashlib.sha256(data).hexdigest()) == recorded[name], name
    path = str(tmp_path / 'none.ply')
    mesh.write_ply(path, v, t, vertex_colors=None, vertex_normals=None)
    assert hashlib.sha256(open(path, 'rb').read()).hexdigest() == recorded['plain'][1]


def test_ply_round_trip_of_normals_and_colours_binary(tmp_path):
    from poseprobe_amd import mesh
    v, t, c = _mesh()
    n = np.random.RandomState(6).randn(7, 3).astype(np.float32)
    path = str(tmp_path / 'a.ply')
    mesh.write_ply(path, v, t, vertex_colors=c, vertex_normals=torch.tensor(n))
    r = mesh.read_ply_attributes(path)
    assert np.array_equal(r['vertices'], v) and np.array_equal(r['triangles'], t) and np.array_equal(r['normals'], n)
    assert r['colors'].dtype == np.uint8 and np.array_equal(r['colors'], np.floor(255 * np.clip(c, 0, 1)).astype(np.uint8))
    v2, t2 = mesh.read_ply(path)                                         # the two-tuple reader skips the attributes
    assert np.array_equal(v2, v) and np.array_equal(t2, t)
    for kw, present in ((dict(vertex_normals=n), ('normals',)), (dict(vertex_colors=c), ('colors',)), ({}, ())):
        mesh.write_ply(path, v, t, **kw)
        r = mesh.read_ply_attributes(path)
        assert [k for k in ('normals', 'colors') if r[k] is not None] == list(present)
        assert np.array_equal(r['vertices'], v) and np.array_equal(r['triangles'], t)
    with pytest.raises(ValueError, match='vertex_normals'):
        mesh.write_ply(path, v, t, vertex_normals=n[:3])


def test_ply_round_trip_of_normals_and_colours_ascii(tmp_path):
    from poseprobe_amd import mesh
    v, t, c = _mesh()
    n = np.random.RandomState(6).randn(7, 3).astype(np.float32)
    c8 = np.floor(255 * c).astype(np.uint8)
    lines = ['ply', 'format ascii 1.0', 'comment written by hand', f'element vertex {len(v)}', 'property float x', 'property float y',
             'property float z', 'property float nx', 'property float ny', 'property float nz', 'property uchar red',
             'property uchar green', 'property uchar blue', f'element face {len(t)}', 'property list uchar int vertex_indices',
             'end_header']
    lines += [' '.join([repr(float(x)) for x in np.concatenate([v[i], n[i]])] + [str(int(x)) for x in c8[i]]) for i in range(len(v))]
    lines += ['3 ' + ' '.join(str(int(x)) for x in row) for row in t]
    path = str(tmp_path / 'ascii.ply')
    open(path, 'w').write('\n'.join(lines) + '\n')
    r = mesh.read_ply_attributes(path)
    assert np.array_equal(r['vertices'], v) and np.array_equal(r['normals'], n) and np.array_equal(r['triangles'], t)
    assert r['colors'].dtype == np.uint8 and np.array_equal(r['colors'], c8)
    assert np.array_equal(mesh.read_ply(path)[0], v)


# ---- the export driver -----------------------------------------------------------------------------------------------------------
def _driver_setup(monkeypatch, tmp_path):
    from poseprobe_amd import dtu_eval, mesh
    v, t, c = _mesh()
    calls = {}

    def extract(model, lo, hi, resolution=128, threshold=0.0, **kw):
        calls['extract'] = dict(model=model, lo=lo, hi=hi, resolution=resolution, threshold=threshold, kw=kw)
        return v.copy(), t.copy()

    def colors(model, vertices, **kw):
        calls['colors'] = dict(model=model, vertices=np.array(vertices), kw=kw)
        return c.copy()

    def score(path, **kw):
        calls['eval'] = dict(path=path, kw=kw)
        return 1.0, 2.0, 1.5

    monkeypatch.setattr(mesh, 'voxurf_extract_deform_geometry', extract)
    monkeypatch.setattr(mesh, 'voxurf_vertex_colors', colors)
    monkeypatch.setattr(dtu_eval, 'eval', score)
    model = types.SimpleNamespace(xyz_min=torch.tensor([-1., -2., -3.]), xyz_max=torch.tensor([1., 2., 3.]))
    cfg = types.SimpleNamespace(basedir=str(tmp_path), expname='exp')
    return dtu_eval, mesh, model, cfg, calls, (v, t, c)


def test_validate_deform_mesh_writes_the_deformed_mesh_under_its_name(monkeypatch, tmp_path):
    dtu_eval, mesh, model, cfg, calls, (v, t, c) = _driver_setup(monkeypatch, tmp_path)
    assert dtu_eval.validate_deform_mesh(model, cfg, resolution=33, threshold=0.25, prefix='_7', smooth=True) == 0.0
    path = os.path.join(str(tmp_path), 'exp', 'meshes', 'deform_7.ply')
    assert os.path.exists(path) and 'colors' not in calls and 'eval' not in calls
    e = calls['extract']
    assert e['model'] is model and e['resolution'] == 33 and e['threshold'] == 0.25
    assert torch.equal(e['lo'], model.xyz_min) and torch.equal(e['hi'], model.xyz_max)
    r = mesh.read_ply_attributes(path)
    assert np.array_equal(r['vertices'], v) and np.array_equal(r['triangles'], t) and r['colors'] is None and r['normals'] is None


def test_validate_deform_mesh_colours_the_unscaled_vertices_and_scales_the_written_ones(monkeypatch, tmp_path):
    dtu_eval, mesh, model, cfg, calls, (v, t, c) = _driver_setup(monkeypatch, tmp_path)
    scale = np.diag([2.5, 2.5, 2.5, 1.0])
    scale[:3, 3] = [10., -20., 30.]
    assert dtu_eval.validate_deform_mesh(model, cfg, world_space=True, scale_mats_np=scale, extract_color=True, global_step=4000,
                                         chunk=3, smooth=False) == 0.0
    assert np.array_equal(calls['colors']['vertices'], v) and calls['colors']['model'] is model
    assert calls['colors']['kw'] == dict(global_step=4000, chunk=3)
    r = mesh.read_ply_attributes(os.path.join(str(tmp_path), 'exp', 'meshes', 'deform.ply'))
    assert np.array_equal(r['vertices'], (v * scale[0, 0] + scale[:3, 3][None]).astype(np.float32))
    assert np.array_equal(r['colors'], np.floor(255 * c).astype(np.uint8))
    # world_space without a matrix, and a matrix without world_space, leave the vertices alone
    for kw in (dict(world_space=True), dict(scale_mats_np=scale)):
        dtu_eval.validate_deform_mesh(model, cfg, prefix='_raw', **kw)
        assert np.array_equal(mesh.read_ply(os.path.join(str(tmp_path), 'exp', 'meshes', 'deform_raw.ply'))[0], v)


def test_validate_deform_mesh_hands_the_file_to_the_score(monkeypatch, tmp_path):
    dtu_eval, mesh, model, cfg, calls, _ = _driver_setup(monkeypatch, tmp_path)
    assert dtu_eval.validate_deform_mesh(model, cfg, prefix='_p', gt_eval=True, scene=24, runtime=False) == 1.5
    mesh_dir = os.path.join(str(tmp_path), 'exp', 'meshes')
    assert calls['eval']['path'] == os.path.join(mesh_dir, 'deform_p.ply')
    assert calls['eval']['kw'] == dict(scene=24, eval_dir=mesh_dir, dataset_dir='data/DTU', suffix='_peval', runtime=False)


def test_validate_mesh_still_refuses_colours():
    from poseprobe_amd import dtu_eval
    with pytest.raises(NotImplementedError, match='extract_color'):
        dtu_eval.validate_mesh(None, None, extract_color=True)


def test_vertex_attributes_refuses_host_tensors_and_other_colour_stages():
    from poseprobe_amd import mesh
    model = types.SimpleNamespace(sdf=types.SimpleNamespace(grid=torch.zeros(1, 1, 2, 2, 2)), k0_dim=12,
                                  rgbnet_kwargs=dict(posbase_pe=5, viewbase_pe=4, rgbnet_width=128))
    with pytest.raises(RuntimeError, match='CUDA'):
        mesh.vertex_attributes(model, torch.zeros(4, 3))
    with pytest.raises(TypeError):
        mesh.vertex_attributes(model, [[0., 0., 0.]])
    with pytest.raises(NotImplementedError, match='viewbase_pe'):
        mesh._color_stage_config(model)


# ---- the C boundary --------------------------------------------------------------------------------------------------------------
def test_the_entry_point_is_declared_and_the_abi_version_stays():
    import ctypes
    from poseprobe_amd import _lib
    protos = _lib.parse_header()
    assert [n for _, n in protos['pp_vertex_feat']] == ['sc', 'sdf_grid', 'sdf_ab', 'k0_cl', 'pts', 'warp_out', 'pe_w', 'n', 'normal',
                                                        'feat', 'stream']
    kinds = [ct for ct, _ in protos['pp_vertex_feat']]
    assert kinds[0] is ctypes.POINTER(_lib.pp_scene) and kinds[7] is ctypes.c_int32
    assert all(k is ctypes.c_void_p for i, k in enumerate(kinds) if i not in (0, 7))
    assert _lib.header_abi_version() == 4
    from poseprobe_amd import ops
    assert callable(ops.vertex_feat)
