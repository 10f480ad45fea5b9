"""Mesh -> signed distance, the parts that need no GPU.  The numpy reference of the GPU tests
(tests/mesh_sdf_reference.py) is checked here against mathematics, never against the code under test: the analytic box, the sphere
and the hollow sphere.  Then the host side of the feature: Voxurf.init_sdf_from_sdf against a float64 restatement of its three
steps (on the CPU, where it runs without the library), the template file's round trip, the grid's node coordinates and the
refusals that are decided before anything is launched."""
import os
import pickle

import numpy as np
import pytest
import torch

from tests import mesh_sdf_reference as R
from poseprobe_amd import mesh


# ---- 1. the reference against mathematics ------------------------------------------------------------------------------------------
def test_reference_box_is_the_analytic_box():
    lo, hi = (2, 1, 3), (6, 5, 6)
    v, t = R.box(lo, hi)
    assert R.odd_edges(t) == 0 and len(t) == 12
    nodes = R.grid_nodes((0, 0, 0), (8, 7, 9), (9, 8, 10))
    want = R.box_sdf(nodes, lo, hi)
    assert int((want == 0).sum()) == 82 and len(want) == 720
    d = R.unsigned_distance(nodes, v, t)[0]
    err = np.abs(d - np.abs(want)).max()
    print(f'box: max |reference - analytic| = {err:.3g}')
    assert err <= 1e-14
    off = want != 0
    assert np.array_equal(R.inside(nodes, v, t)[off], want[off] < 0)
    # generic nodes as well: none on the surface, every sign compared
    nodes = R.grid_nodes((0.13, 0.21, 0.07), (7.9, 6.8, 8.7), (10, 9, 11))
    want = R.box_sdf(nodes, lo, hi)
    got = R.signed_distance(nodes, v, t)
    assert np.abs(got - want).max() <= 1e-14 and (want < 0).sum() > 20


@pytest.mark.parametrize('shape', ['sphere', 'hollow'])
def test_reference_sphere_within_the_hausdorff_distance_of_its_polyhedron(shape):
    centre, r = np.array([12.3, 10.1, 11.4]), 8.37
    nodes = R.grid_nodes((0, 0, 0), (24, 20, 22), (13, 11, 9)).astype(np.float64)
    rad = np.linalg.norm(nodes - centre[None], axis=1)
    if shape == 'sphere':
        v, t = R.sphere(2, r, centre)
        want = rad - r
        slack = r - R.smallest_face_distance(v, t, centre)
    else:
        r_in = 4.5
        v, t = R.nested_spheres(2, r, r_in, centre)
        want = np.maximum(rad - r, r_in - rad)
        n_outer = len(t) // 2
        slack = max(r - R.smallest_face_distance(v, t[:n_outer], centre), r_in - R.smallest_face_distance(v, t[n_outer:], centre))
    assert R.odd_edges(t) == 0
    slack += 4 * R.ulp32(r + np.abs(centre).max())                              # the vertices are float32
    got = R.signed_distance(nodes, v, t)
    print(f'{shape}: r - rho = {slack:.4g}, max |reference - analytic| = {np.abs(got - want).max():.4g}')
    assert np.abs(got - want).max() <= slack
    clear = np.abs(want) > slack
    assert clear.sum() > 0.8 * len(want) and np.array_equal(got[clear] < 0, want[clear] < 0)
    if shape == 'hollow':
        assert (got[rad < r_in - slack] > 0).all() and (rad < r_in - slack).sum() >= 4       # the cavity is outside


def test_reference_takes_a_triangle_without_area_as_a_segment():
    v = np.array([[0, 0, 0], [2, 0, 0], [1, 0, 0], [5, 5, 5]], np.float32)
    t = np.array([[0, 1, 2], [3, 3, 3]], np.int32)                              # a segment from (0,0,0) to (2,0,0), and a point
    p = np.array([[1, 3, 0], [-1, 0, 0], [3, 4, 0], [5, 5, 7]], np.float64)
    d, c, i = R.unsigned_distance(p, v, t)
    assert np.allclose(d, [3, 1, np.sqrt(17), 2], atol=1e-15) and i.tolist() == [0, 0, 0, 1]
    assert np.allclose(c, [[1, 0, 0], [0, 0, 0], [2, 0, 0], [5, 5, 5]], atol=1e-15)
    assert not R.inside(p, v, t).any()


def test_reference_tolerance_has_its_floor_at_four_ulps_of_the_largest_coordinate():
    v, t = R.box((2, 1, 3), (6, 5, 6))
    nodes = R.grid_nodes((0, 0, 0), (8, 7, 9), (9, 8, 10))
    tol, dev = R.tolerance(nodes, v, t)
    print(f'box: float32 restatement deviates by {dev:.3g}, tolerance {tol:.3g}')
    assert tol == max(4 * dev, 4 * R.ulp32(9.0)) and dev < 4e-6


# ---- 2. init_sdf_from_sdf ----------------------------------------------------------------------------------------------------------------
def _model(G=8, **kw):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd import voxurf_coarse as Model
    rs = syn.range_shape()
    args = dict(num_voxels=G ** 3, num_voxels_base=G ** 3, alpha_init=1e-2, rgbnet_dim=12, rgbnet_direct=True, rgbnet_depth=4,
                rgbnet_width=128, posbase_pe=5, viewbase_pe=1, geo_rgb_dim=3, s_ratio=50, s_start=0.2, barf_c2f=[0.6, 1],
                i_train=np.arange(3), N_iters=10000, HW=np.array([[8, 8]] * 3), range_shape=rs, rect_size=rs.tolist(), camera_noise=0.)
    args.update(kw)
    return Model.Voxurf(syn.XYZ_MIN, syn.XYZ_MAX, **args)


@pytest.mark.parametrize('smooth,reduce,shape,ksize,sigma', [(False, 1.0, 'same', 3, 1.0), (False, 2.5, 'same', 3, 1.0),
                                                             (False, 1.0, 'other', 3, 1.0), (True, 1.0, 'same', 3, 1.0),
                                                             (True, 2.0, 'same', 3, 1.0), (True, 1.5, 'other', 5, 0.8)])
def test_init_sdf_from_sdf_equals_the_float64_restatement(smooth, reduce, shape, ksize, sigma):
    m = _model()
    ws = tuple(int(s) for s in m.world_size.tolist())
    assert tuple(m.sdf.grid.shape[2:]) == ws
    src = ws if shape == 'same' else (ws[0] + 3, ws[1] - 2, ws[2] + 5)
    sdf0 = np.random.RandomState(3).randn(*src).astype(np.float32)
    m.init_sdf_from_sdf(torch.from_numpy(sdf0.copy())[None, None], smooth=smooth, reduce=reduce, ksize=ksize, sigma=sigma)
    want = R.init_sdf_from_sdf(sdf0, ws, smooth=smooth, reduce=reduce, ksize=ksize, sigma=sigma)
    got = m.sdf.grid.detach()[0, 0].numpy()
    assert got.shape == ws and got.dtype == np.float32
    err = np.abs(got - want).max()
    print(f'smooth={smooth} reduce={reduce} {shape}: max err {err:.3g}')
    if not smooth and shape == 'same' and reduce == 1.0:
        assert np.array_equal(got, sdf0)                                        # the bits that came in
    assert err <= 32 * R.ulp32(np.abs(sdf0).max())                              # a few dozen float32 roundings in the resize and the 125-tap sum
    if smooth and reduce != 1.0:                                                # the reference divides twice: once would be `reduce` times larger
        assert np.abs(got * reduce - want).max() > 0.1 * np.abs(want).max()
    assert not m.sdf.grid.requires_grad and isinstance(m.sdf.grid, torch.nn.Parameter)
    assert 'sdf.grid' in m.state_dict()


def test_init_sdf_from_sdf_refuses_what_is_no_grid():
    m = _model()
    with pytest.raises(ValueError):
        m.init_sdf_from_sdf(torch.zeros(8, 8, 8))
    with pytest.raises(ValueError):
        m.init_sdf_from_sdf(np.zeros((1, 1, 8, 8, 8), np.float32))


def test_smoothing_at_render_time_is_still_refused():
    with pytest.raises(NotImplementedError):
        _model(smooth_ksize=3)


# ---- 3. the template file and the nodes ---------------------------------------------------------------------------------------------------
def test_template_file_round_trip_in_the_format_of_the_mask_cache(tmp_path):
    sdf = np.random.RandomState(1).randn(5, 4, 6).astype(np.float32)
    lo, hi = np.array([-0.6, -0.6, -0.7], np.float32), np.array([0.6, 0.6, 0.5], np.float32)
    path = os.path.join(tmp_path, 'template.pkl')
    mesh.save_sdf_grid(path, torch.from_numpy(sdf.copy())[None, None], torch.from_numpy(lo), hi)
    with open(path, 'rb') as f:
        raw = pickle.load(f)                                                    # lib/voxurf_coarse.py:1271-1282 reads exactly these keys
    assert set(raw) == {'sdf_grid_xyz', 'xyz_min', 'xyz_max'} and isinstance(raw['sdf_grid_xyz'], np.ndarray)
    g, a, b = mesh.load_sdf_grid(path)
    assert np.array_equal(g, sdf) and g.dtype == np.float32 and np.array_equal(a, lo) and np.array_equal(b, hi)
    with open(path, 'wb') as f:
        pickle.dump({'sdf_grid_xyz': sdf}, f)
    with pytest.raises(ValueError):
        mesh.load_sdf_grid(path)


def test_nodes_sit_where_cube_sdf_puts_them():
    lo, hi, ws = (-0.6, -0.6, -0.7), (0.6, 0.6, 0.5), (24, 18, 30)
    axes = mesh.sdf_grid_axes(np.array(lo, np.float32), torch.tensor(hi), ws)
    x, y, z = np.mgrid[lo[0]:hi[0]:ws[0] * 1j, lo[1]:hi[1]:ws[1] * 1j, lo[2]:hi[2]:ws[2] * 1j]
    for got, want, ref in zip(axes, (x[:, 0, 0], y[0, :, 0], z[0, 0, :]), R.grid_axes(np.float32(lo), np.float32(hi), ws)):
        assert got.dtype == np.float32 and np.array_equal(got, ref)
        assert np.abs(got - want).max() <= 2 * R.ulp32(0.7)                     # (np.mgrid starts from the float64 literals)
    with pytest.raises(ValueError):
        mesh.sdf_grid_axes(lo, hi, (24, 0, 30))
    with pytest.raises(ValueError):
        mesh.sdf_grid_axes(lo, lo, ws)
    with pytest.raises(ValueError):
        mesh.sdf_grid_axes((1e8, 0, 0), (1e8 + 1, 1, 1), (64, 4, 4))           # float32 cannot tell these nodes apart


# ---- 4. refusals decided on the host ------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_the_device_is_touched():
    v, t = R.box((2, 1, 3), (6, 5, 6))
    box = ((0, 0, 0), (8, 7, 9), (9, 8, 10))
    with pytest.raises(TypeError):
        mesh.signed_distance_grid(v, t.astype(np.float32), *box)
    with pytest.raises(TypeError):
        mesh.signed_distance_grid(v.astype(np.int32), t, *box)
    with pytest.raises(ValueError):
        mesh.signed_distance_grid(v[:, :2], t, *box)
    with pytest.raises(ValueError):
        mesh.signed_distance_grid(v, t, (0, 0, 0), (8, 7, 9), (9, 8))
    with pytest.raises(RuntimeError):
        mesh.signed_distance_grid(torch.from_numpy(v), torch.from_numpy(t), *box)        # CPU tensors
    with pytest.raises(RuntimeError):
        mesh.unsigned_distance(torch.zeros(4, 3), v, t)
    with pytest.raises(ValueError):
        mesh.unsigned_distance(np.zeros((4, 2), np.float32), v, t)


def test_odd_edge_count_equals_the_restated_count():
    v, t = R.box((0, 0, 0), (1, 1, 1))
    cases = {'closed': t, 'minus one': t[1:], 'minus a face': t[2:], 'doubled': np.concatenate([t, t]),
             'repeated vertex': np.concatenate([t, [[0, 0, 5]]]).astype(np.int32)}
    want = {'closed': 0, 'minus one': 3, 'minus a face': 4, 'doubled': 0, 'repeated vertex': 0}
    for name, tri in cases.items():
        assert R.odd_edges(tri) == want[name], name
        assert mesh.odd_edge_count(torch.from_numpy(np.array(tri))) == want[name], name
