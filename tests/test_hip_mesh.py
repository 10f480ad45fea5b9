"""Mesh extraction on the GPU (poseprobe_amd.mesh, csrc/pp_mesh.hip) against the numpy restatement of its semantics
(tests/mesh_reference.py, itself checked against mathematics in tests/test_mesh_host.py): parity index by index on the
smallest lattices and on one that spans many tiles, properties of the device output, the device field fill, and the
model-level entry points end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_reference as R
from tests.helpers import assert_close, load

pytestmark = pytest.mark.gpu


def _tiny(shape, seed):
    return R.noise_field(shape, seed=seed)


FIELDS = {                               # name: (field builder, threshold)
    'noise_2x2x2': (lambda: _tiny((2, 2, 2), 3), 0.0),
    'noise_2x3x2': (lambda: _tiny((2, 3, 2), 4), 0.0),
    'noise_3x2x5': (lambda: _tiny((3, 2, 5), 5), 0.0),
    'sphere': (R.sphere_field, 0.0),
    'torus': (R.torus_field, 0.0),
    'plane': (R.plane_field, 0.0),
    'all_above': (lambda: np.full((4, 3, 5), 1.0, np.float32), 0.0),
    'all_below': (lambda: np.full((4, 3, 5), -1.0, np.float32), 0.0),
    'noise_20': (lambda: R.noise_field((20, 20, 20), seed=0), 0.0),
    'noise_closed': (lambda: R.noise_field((14, 13, 12), closed=True), 0.0),
    # a positive field and the threshold DirectVoxGO's density mode uses
    'positive_0.001': (lambda: (np.random.RandomState(7).rand(9, 7, 11) * 0.004).astype(np.float32), 0.001),
    # odd sizes, 600 tiles of 1024 points, x stride of 4690 points: tile borders cut rows, planes and the surface
    'big': (R.big_field, 0.0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(field, threshold, reference vertices, reference triangles) - computed once, read-only."""
    build, thr = FIELDS[name]
    u = build()
    v, t = R.marching_cubes(u, thr)
    for a in (u, v, t):
        a.setflags(write=False)
    return u, thr, v, t


def assert_mesh_equal(vertices, triangles, v_ref, t_ref, extent, name=''):
    """Triangles as integer arrays; vertices within 2^-20 x the lattice extent (they are expected to be bit-equal: the compare,
    the subtractions, the correctly rounded division and the addition are the same fp32 operations on both sides)."""
    t = triangles.cpu().numpy() if isinstance(triangles, torch.Tensor) else triangles
    v = vertices.cpu().numpy() if isinstance(vertices, torch.Tensor) else vertices
    assert v.dtype == np.float32 and t.dtype == np.int32
    assert v.shape == v_ref.shape and t.shape == t_ref.shape, (name, v.shape, v_ref.shape, t.shape, t_ref.shape)
    assert np.array_equal(t, t_ref), f'{name}: triangles differ'
    diff = float(np.abs(v.astype(np.float64) - v_ref).max()) if v.size else 0.0
    print(f'{name}: {len(v)} vertices, {len(t)} triangles, max |dv| = {diff:.3e}, bit-equal: {np.array_equal(v, v_ref)}')
    assert diff <= 2.0 ** -20 * extent, f'{name}: vertices differ by {diff:.3e}'


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(FIELDS))
def test_marching_cubes_matches_the_reference(name):
    from poseprobe_amd import mesh
    u, thr, v_ref, t_ref = case(name)
    v, t = mesh.marching_cubes(torch.tensor(u, device='cuda'), thr)
    assert v.is_cuda and t.is_cuda and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    assert_mesh_equal(v, t, v_ref, t_ref, max(u.shape), name)
    if name == 'noise_20':
        assert len(np.unique(R.case_index(u, thr))) == 256          # every table row is exercised
    if name.startswith('all_'):
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_marching_cubes_uploads_numpy_fields():
    from poseprobe_amd import mesh
    u, thr, v_ref, t_ref = case('noise_3x2x5')
    v, t = mesh.marching_cubes(np.asarray(u, dtype=np.float64), thr)
    assert_mesh_equal(v, t, v_ref, t_ref, max(u.shape), 'numpy input')


# ---- 2. properties of the device output ----------------------------------------------------------------------------------------
def test_device_sphere_is_a_closed_outward_oriented_manifold():
    from poseprobe_amd import mesh
    u, thr, _, _ = case('sphere')
    v, t = mesh.marching_cubes(torch.tensor(u, device='cuda'), thr)
    R.sphere_checks(v.cpu().numpy(), t.cpu().numpy())


def test_two_runs_give_identical_bits():
    from poseprobe_amd import mesh
    u = torch.tensor(case('big')[0], device='cuda')
    a, b = mesh.marching_cubes(u, 0.0), mesh.marching_cubes(u, 0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].data_ptr() != b[0].data_ptr()


@pytest.mark.parametrize('name', ['noise_3x2x5', 'sphere', 'big'])
def test_emit_writes_the_counted_rows_and_the_workspace_it_asked_for_only(name):
    """Guard rows behind the outputs and guard bytes behind the workspace stay untouched; one byte less is refused."""
    from poseprobe_amd import _lib, ops
    u_h, thr, v_ref, t_ref = case(name)
    u = torch.tensor(u_h, device='cuda')
    need = ops.mc_workspace(*u.shape)
    guard = 4096
    arena = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device='cuda')
    work = arena[:need]
    counts = torch.full((2,), -1, dtype=torch.int32, device='cuda')
    ops.mc_count(u, thr, work, counts)
    nv, nt = counts.tolist()
    assert (nv, nt) == (len(v_ref), len(t_ref))
    vertices = torch.full((nv + 8, 3), 7.0, device='cuda')
    triangles = torch.full((nt + 8, 3), -7, dtype=torch.int32, device='cuda')
    ops.mc_emit(u, thr, work, vertices, nv, triangles, nt)
    torch.cuda.synchronize()
    assert bool((vertices[nv:] == 7.0).all()) and bool((triangles[nt:] == -7).all())
    assert bool((arena[need:] == 0xA5).all())
    assert_mesh_equal(vertices[:nv], triangles[:nt], v_ref, t_ref, max(u.shape), name)
    for call in (lambda w: ops.mc_count(u, thr, w, counts), lambda w: ops.mc_emit(u, thr, w, vertices, nv, triangles, nt)):
        with pytest.raises(_lib.PoseProbeError, match='workspace too small'):
            call(arena[:need - 1])
    with pytest.raises(RuntimeError, match='rows'):
        ops.mc_emit(u, thr, work, vertices[:nv], nv + 1, triangles, nt)


# ---- 3. field fill ---------------------------------------------------------------------------------------------------------------
LO, HI = [-1., -0.5, 0.], [1., 0.5, 2.]


@pytest.mark.parametrize('resolution,N', [(5, 2), (7, 3), (6, 3), (4, 64)])
def test_extract_fields_device_walks_the_lattice_like_extract_fields(resolution, N):
    from poseprobe_amd import dvgo_ori, mesh
    f = lambda p: p.sum(-1)
    ref = dvgo_ori.extract_fields(torch.tensor(LO), torch.tensor(HI), resolution, f, N)
    got = mesh.extract_fields_device(torch.tensor(LO), torch.tensor(HI), resolution, f, N)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    # the same fp32 lattice points on both sides; a three-term fp32 sum in either association: 2 ulp of a partial sum below 4
    assert_close(got, ref, rtol=0, atol=2.0 ** -21, name='p.sum(-1) on the lattice')


@functools.lru_cache(maxsize=None)
def voxurf_g24():
    from tests.test_hip_dropin import make_model
    return make_model(load('inference_g24.npz')).eval()


def _lattice(m, resolution):
    lo, hi = m.xyz_min.cpu(), m.xyz_max.cpu()
    axes = [torch.linspace(float(lo[a]), float(hi[a]), resolution) for a in range(3)]
    return lo, hi, torch.stack(torch.meshgrid(*axes, indexing='ij'), dim=-1).reshape(-1, 3)


def _sample_border(grid, pts, lo, hi):
    """grid_sampler of lib/voxurf_coarse.py:522-543 (bilinear, align_corners, border padding) in torch on the CPU."""
    import torch.nn.functional as F
    ind = ((pts.reshape(1, 1, 1, -1, 3) - lo) / (hi - lo)).flip((-1,)) * 2 - 1
    return F.grid_sample(grid.contiguous(), ind, mode='bilinear', align_corners=True, padding_mode='border').reshape(-1)


def test_voxurf_plain_field_matches_torch_grid_sample():
    from poseprobe_amd import mesh
    m, res = voxurf_g24(), 33
    lo, hi, pts = _lattice(m, res)
    got = mesh.extract_fields_device(lo, hi, res, mesh.voxurf_field(m), N=16, device='cuda')
    ref = _sample_border(-m.sdf.grid.detach().cpu(), pts, lo, hi).reshape(res, res, res)
    assert_close(got, ref, rtol=1e-5, atol=1e-6, name='-sdf on the lattice')


def test_voxurf_deform_field_matches_a_torch_restatement():
    """-(mapped template at the warped point + correction), lib/voxurf_coarse.py:1224-1240, from the model's own parameters."""
    import torch.nn.functional as F
    from poseprobe_amd import mesh
    from tests.test_hip_mlp import _close_but_flipped_rows
    m, res = voxurf_g24(), 33
    lo, hi, pts = _lattice(m, res)
    got = mesh.extract_fields_device(lo, hi, res, mesh.voxurf_deform_field(m), N=20, device='cuda')
    with torch.no_grad():
        h = pts
        lins = m.warp_network.linears()
        for i, lin in enumerate(lins):
            h = F.linear(h, lin.weight.cpu(), lin.bias.cpu())
            if i < len(lins) - 1:
                h = F.relu(h)
        out = h * m.warp_network.output_range
        sp = lambda t: F.softplus(t.detach().cpu(), beta=10)
        mapped = sp(m.sdf_alpha) * (torch.sigmoid(sp(m.sdf_beta) * m.sdf.grid.detach().cpu()) - 0.5)
        ref = -(_sample_border(mapped, pts + out[:, :3], lo, hi) + out[:, 3])
    _close_but_flipped_rows(got.reshape(-1, 1).cpu().numpy(), ref.reshape(-1, 1).numpy(), rtol=1e-4, atol=1e-5,
                            name='-sdf_final on the lattice', max_rows=3)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
def _world(v, resolution, lo, hi):
    """lib/dvgo_ori.py:699-702."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return v / (resolution - 1.0) * (hi - lo)[None, :] + lo[None, :]


@pytest.mark.parametrize('deform', [False, True])
def test_voxurf_geometry_end_to_end(deform):
    from poseprobe_amd import mesh
    m, res = voxurf_g24(), 33
    lo, hi = m.xyz_min, m.xyz_max
    extract, field = ((mesh.voxurf_extract_deform_geometry, mesh.voxurf_deform_field) if deform else
                      (mesh.voxurf_extract_geometry, mesh.voxurf_field))
    vertices, triangles = extract(m, lo, hi, resolution=res, threshold=0.0, scale_mats_np=None, gt_path=None, smooth=False)
    assert isinstance(vertices, np.ndarray) and isinstance(triangles, np.ndarray) and len(triangles) > 0
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    slack = 4 * np.finfo(np.float32).eps * np.abs(np.stack([lo_h, hi_h])).max()       # fp32 rounding of the world transform
    assert (vertices >= lo_h - slack).all() and (vertices <= hi_h + slack).all()
    # the same device field through the reference: the MLP's precision does not enter
    u = mesh.extract_fields_device(lo, hi, res, field(m), device='cuda').cpu().numpy()
    v_ref, t_ref = R.marching_cubes(u, 0.0)
    assert np.array_equal(triangles, t_ref)
    assert_close(vertices, _world(v_ref, res, lo_h, hi_h), rtol=0, atol=2.0 ** -20 * float((hi_h - lo_h).max()), name='world vertices')
    none_res = extract(m, lo, hi, resolution=None)
    assert len(none_res[1]) > 0                                       # resolution=None: world_size[0]


def test_extract_geometry_world_transform():
    from poseprobe_amd import mesh
    res = 21
    lo, hi = torch.tensor([-1.0, 0.5, 2.0]), torch.tensor([3.0, 1.5, 2.5])
    c, r = torch.tensor([1.1, 1.0, 2.25]), 0.4
    field = lambda p: r - ((p - c.to(p.device)) / torch.tensor([4.0, 1.0, 0.4], device=p.device)).norm(dim=-1)
    vertices, triangles = mesh.extract_geometry(lo, hi, res, 0.0, field, N=8)
    lattice = mesh.extract_fields_device(lo, hi, res, field, N=8).cpu().numpy()
    v_lat, t_lat = R.marching_cubes(lattice, 0.0)
    assert len(t_lat) > 0 and np.array_equal(triangles, t_lat)
    assert_close(vertices, _world(v_lat, res, lo.numpy(), hi.numpy()), rtol=0, atol=2.0 ** -20 * 4.0, name='world vertices')


def test_dvgo_density_geometry_runs_on_the_twin():
    from poseprobe_amd import mesh
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.dvgo_ori import DirectVoxGO
    d = load('dvgo_g16.npz')
    G = int(d['G'])
    m = DirectVoxGO(syn.XYZ_MIN, syn.XYZ_MAX, num_voxels=G ** 3, num_voxels_base=G ** 3, alpha_init=1e-2, rgbnet_dim=12,
                    rgbnet_direct=True, rgbnet_depth=3, rgbnet_width=128, posbase_pe=5, viewbase_pe=4, fast_color_thres=1e-4)
    sd = m.state_dict()
    sd['density'], sd['k0'] = torch.tensor(d['density']), torch.tensor(d['k0'])
    m.load_state_dict(sd)
    m = m.cuda()
    res = 19
    vertices, triangles = mesh.dvgo_extract_geometry(m, m.xyz_min, m.xyz_max, resolution=res, threshold=0.5, mode='density')
    query, thr = mesh.dvgo_field(m, 'density')
    assert thr == 0.001                                               # forced, whatever the caller passed (lib/dvgo_ori.py:384)
    u = mesh.extract_fields_device(m.xyz_min, m.xyz_max, res, query).cpu().numpy()
    v_ref, t_ref = R.marching_cubes(u, thr)
    assert np.array_equal(triangles, t_ref) and vertices.shape == v_ref.shape
    assert_close(vertices, _world(v_ref, res, m.xyz_min.cpu().numpy(), m.xyz_max.cpu().numpy()), rtol=0,
                 atol=2.0 ** -20 * float((m.xyz_max - m.xyz_min).max()), name='world vertices')
    with pytest.raises(NotImplementedError, match='neus'):
        mesh.dvgo_extract_geometry(m, m.xyz_min, m.xyz_max, resolution=res, mode='neus')
