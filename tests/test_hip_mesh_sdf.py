"""Mesh -> signed distance on the GPU (poseprobe_amd.mesh.unsigned_distance / signed_distance_grid / voxurf_template_from_mesh,
csrc/pp_mesh_sdf.hip) against the numpy float64 reference (tests/mesh_sdf_reference.py, itself checked against
mathematics in tests/test_mesh_sdf_host.py).

Tolerance of a case: 4 x the largest deviation of the reference's own float32 restatement from float64 on that case, and no less
than 4 float32 ulps of the largest coordinate in play - computed at run time and printed.  Signs are compared at every node whose
float64 |d| exceeds the tolerance, magnitudes everywhere; at most 1 % of a generic case may lie below it (the box case leaves
nothing out: its 82 surface nodes must come out 0 within the tolerance).  The shapes are the smallest at which each mechanism can
still go wrong."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_sdf_reference as R

pytestmark = pytest.mark.gpu

CENTRE = (12.3, 10.1, 11.4)
GENERIC = {
    # name: (mesh, xyz_min, xyz_max, world_size)
    'sphere': (lambda: R.sphere(2, 8.37, CENTRE), (0, 0, 0), (24, 20, 22), (13, 11, 9)),
    'sphere_cut': (lambda: R.sphere(2, 8.37, CENTRE), (0, 0, 6), (24, 20, 17), (13, 11, 9)),       # the mesh pokes out of the grid in z
    'torus': (lambda: R.torus(24, 12, 6.3, 2.4, (10.2, 9.7, 4.9)), (0, 0, 0), (20.5, 19.5, 10), (17, 15, 12)),
    'nested': (lambda: R.nested_spheres(2, 8.5, 4.5, CENTRE), (0, 0, 0), (24.6, 20.2, 22.8), (13, 11, 12)),
}
BOX = ((2, 1, 3), (6, 5, 6))
BOX_GRID = ((0, 0, 0), (8, 7, 9), (9, 8, 10))
FAR_GRID = ((0, 0, 0), (39, 2, 2), (40, 3, 3))


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(v, t, grid, nodes, ref: signed float64 reference at the nodes, tol, dev) - computed once, read-only."""
    if name in GENERIC:
        make, *grid = GENERIC[name]
        v, t = make()
    elif name == 'box':
        (v, t), grid = R.box(*BOX), BOX_GRID
    elif name == 'far':
        (v, t), grid = R.tetrahedron((1.3, 1.1, 0.9), 0.6), FAR_GRID
    nodes = R.grid_nodes(*grid)
    d64 = R.unsigned_distance(nodes, v, t)[0]
    ref = R.box_sdf(nodes, *BOX) if name == 'box' else np.where(R.inside(nodes, v, t), -d64, d64)
    tol, dev = R.tolerance(nodes, v, t, d64)
    frozen(v, t, nodes, ref)
    return dict(v=v, t=t, grid=tuple(grid), nodes=nodes, ref=ref, tol=tol, dev=dev)


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(device='cuda', dtype=dtype)             # (a copy: the cases are read-only)


def check_grid(name, got, c, max_near=0.01):
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(c['grid'][2])
    g, ref, tol = got.cpu().numpy().reshape(-1).astype(np.float64), c['ref'], c['tol']
    err = np.abs(np.abs(g) - np.abs(ref)).max()
    clear = np.abs(ref) > tol
    wrong = int(((g[clear] < 0) != (ref[clear] < 0)).sum())
    print(f'{name}: float32 restatement deviates by {c["dev"]:.3g}, tolerance {tol:.3g}; max magnitude error {err:.3g}; '
          f'{int((~clear).sum())} of {len(ref)} nodes below the tolerance; {wrong} wrong signs; {int((ref < -tol).sum())} nodes inside')
    assert np.isfinite(g).all()
    assert err <= tol
    assert wrong == 0
    assert (~clear).sum() <= max_near * len(ref)


# ---- 1. generic position ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(GENERIC))
def test_generic_position_value_and_sign_at_every_node(name):
    from poseprobe_amd import mesh
    c = case(name)
    info = {}
    got = mesh.signed_distance_grid(c['v'], c['t'], *c['grid'], info=info)
    print(name, info)
    assert (c['ref'] < -c['tol']).sum() >= 20 and info['pairs'] >= len(c['t']) and info['rings_mean'] >= 1
    check_grid(name, got, c)
    if name == 'nested':                                                            # the cavity is outside
        rad = np.linalg.norm(c['nodes'].astype(np.float64) - np.array(CENTRE)[None], axis=1)
        cavity = torch.from_numpy(rad < 4.0).cuda()
        assert int(cavity.sum()) >= 8 and bool((got.reshape(-1)[cavity] > 0).all())


# ---- 2. degenerate position --------------------------------------------------------------------------------------------------------------
def test_box_with_faces_in_node_planes_equals_the_analytic_box():
    from poseprobe_amd import mesh
    c = case('box')
    on = c['ref'] == 0
    assert int(on.sum()) == 82 and len(on) == 720
    got = mesh.signed_distance_grid(c['v'], c['t'], *c['grid'])
    check_grid('box', got, c, max_near=82 / 720)
    g = got.cpu().numpy().reshape(-1).astype(np.float64)
    assert np.abs(g[on]).max() <= c['tol']                                          # on the surface: 0, of either sign
    assert np.abs(g - c['ref']).max() <= c['tol']                                   # everywhere else |d| >= 1: value AND sign
    assert int((g[~on] < 0).sum()) == int((c['ref'] < 0).sum()) == 3 * 3 * 2


# ---- 3. far queries --------------------------------------------------------------------------------------------------------------------
def test_far_nodes_and_points_outside_the_cell_grid():
    from poseprobe_amd import mesh
    c = case('far')
    coarse, fine = {}, {}
    got = mesh.signed_distance_grid(c['v'], c['t'], *c['grid'], info=coarse)
    check_grid('far', got, c)
    again = mesh.signed_distance_grid(c['v'], c['t'], *c['grid'], info=fine, cell_edge=0.2)    # the tetrahedron spans 6 cells an axis
    print('far:', coarse, fine)
    assert torch.equal(got, again) and fine['pairs'] > coarse['pairs'] and fine['rings_max'] > coarse['rings_max'] >= 1
    assert fine['rings_max'] <= max(fine['cells']) + 1                              # a far query ends where the cells end
    p = np.array([[-50, 30, 10], [1.3, 1.1, 300], [80, -2, 0.5], [1.2, 1.0, 0.8], [2.5, 1.1, 0.9], [0, 0, 0]], np.float32)
    want = R.unsigned_distance(p, c['v'], c['t'])[0]
    tol = R.tolerance(p, c['v'], c['t'], want)[0]
    for edge in (None, 0.2, 0.05):
        info = {}
        d, closest, tri = mesh.unsigned_distance(p, c['v'], c['t'], cell_edge=edge, info=info)
        print(f'points, cell_edge={edge}: {info}; max error {np.abs(d.cpu().numpy() - want).max():.3g}, tolerance {tol:.3g}')
        assert np.abs(d.cpu().numpy() - want).max() <= tol
        if edge is None:
            first = (d, closest, tri)
        else:
            assert all(torch.equal(a, b) for a, b in zip(first, (d, closest, tri)))                # whatever the cell grid


def test_max_dist_caps_the_search():
    from poseprobe_amd import mesh
    c = case('torus')
    want = np.abs(c['ref'])
    cap = 3.0
    d, closest, tri = mesh.unsigned_distance(c['nodes'], c['v'], c['t'], max_dist=cap)
    d, tri = d.cpu().numpy(), tri.cpu().numpy()
    near, far = want < cap - c['tol'], want > cap + c['tol']
    assert near.sum() > 100 and far.sum() > 100
    assert np.abs(d[near] - want[near]).max() <= c['tol'] and (tri[near] >= 0).all()
    assert np.isinf(d[far]).all() and (tri[far] == -1).all() and torch.isnan(closest[torch.from_numpy(far).cuda()]).all()
    with pytest.raises(ValueError):
        mesh.unsigned_distance(c['nodes'], c['v'], c['t'], max_dist=0.0)


# ---- 4. binning ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def odd_mesh():
    """A small tetrahedron, one triangle across the whole box (its bounding box is every cell), a triangle without area that is a
    segment, one that is a point, a duplicate of a vertex and two vertices nothing references."""
    v, t = R.tetrahedron((2.2, 1.9, 2.4), 0.5)
    extra = np.array([[0.1, 0.2, 0.1], [7.9, 0.3, 8.8], [4.2, 6.9, 4.1],            # 4 5 6: the diagonal triangle
                      [6.0, 5.0, 1.0], [7.0, 6.0, 2.0], [6.5, 5.5, 1.5],            # 7 8 9: collinear
                      [1.0, 6.0, 8.0],                                              # 10: a point
                      [50.0, 50.0, 50.0], [-9.0, 3.0, 3.0]], np.float32)           # 11 12: unreferenced
    v = np.concatenate([v, extra, v[:1]])                                           # 13: a duplicate of vertex 0
    t = np.concatenate([t, [[4, 5, 6], [7, 8, 9], [10, 10, 10], [13, 1, 2]]]).astype(np.int32)
    return frozen(v, t)


def check_self_consistent(q, v, t, d, closest, tri, tol):
    """The returned closest point lies on the returned triangle, and its distance to the query is the returned distance."""
    q, v = np.asarray(q, np.float64), np.asarray(v, np.float64)
    d, closest, tri = d.cpu().numpy().astype(np.float64), closest.cpu().numpy().astype(np.float64), tri.cpu().numpy()
    assert tri.min() >= 0 and tri.max() < len(t)
    a, b, c = (v[t[tri, k]] for k in range(3))
    assert np.abs(np.linalg.norm(q - closest, axis=1) - d).max() <= tol
    on = np.concatenate([np.diagonal(R.closest_on_triangles(closest[s:s + 256, None], a[None, s:s + 256], b[None, s:s + 256],
                                                            c[None, s:s + 256]), axis1=0, axis2=1).T for s in range(0, len(q), 256)])
    assert np.abs(on - closest).max() <= tol                                        # off the triangle by no more than the tolerance
    n = np.cross(b - a, c - a)
    proper = (n * n).sum(1) > 0
    if proper.any():                                                                # barycentric coordinates in [0, 1] within the tolerance
        ab, ac, ap = (b - a)[proper], (c - a)[proper], (closest - a)[proper]
        nn = (n[proper] ** 2).sum(1)
        bv = (np.cross(ap, ac) * n[proper]).sum(1) / nn
        bw = (np.cross(ab, ap) * n[proper]).sum(1) / nn
        slack = tol / np.sqrt(nn) * np.maximum(np.linalg.norm(ab, axis=1), np.linalg.norm(ac, axis=1))     # tol over the triangle's height
        assert (bv >= -slack).all() and (bw >= -slack).all() and (bv + bw <= 1 + slack).all()


def test_binning_a_triangle_in_every_cell_duplicates_and_triangles_without_area():
    from poseprobe_amd import mesh
    v, t = odd_mesh()
    nodes = R.grid_nodes((0, 0, 0), (8, 7, 9), (7, 6, 5))
    want, _, _ = R.unsigned_distance(nodes, v, t)
    tol, deviation = R.tolerance(nodes, v, t, want)
    results = []
    for edge in (None, 1.0, 0.5):
        info = {}
        d, closest, tri = mesh.unsigned_distance(dev(nodes), dev(v), dev(t), cell_edge=edge, info=info)
        err = np.abs(d.cpu().numpy() - want).max()
        print(f'cell_edge={edge}: {info}; deviation {deviation:.3g}, tolerance {tol:.3g}, max error {err:.3g}')
        assert err <= tol
        check_self_consistent(nodes, v, t, d, closest, tri, tol)
        results.append((d, closest, tri))
    assert all(torch.equal(x, y) for r in results[1:] for x, y in zip(results[0], r))
    assert info['pairs'] >= np.prod(info['cells'])                                  # the diagonal triangle alone is in every cell
    hit = set(results[0][2].cpu().numpy().tolist())
    assert {4, 5, 6} <= hit                                                         # the big one, the segment and the point are each nearest somewhere
    # a triangle without area changes no sign: the box plus a segment (p, q, q), which has no odd edge
    bv, bt = R.box(*BOX)
    v2 = np.concatenate([bv, [[4.0, 3.0, 4.5], [7.5, 6.5, 8.5]]]).astype(np.float32)                     # from inside the box to outside
    t2 = np.concatenate([bt, [[8, 9, 9]]]).astype(np.int32)
    lo, hi, ws = (0.2, 0.1, 0.3), (7.9, 6.8, 8.9), (9, 8, 10)
    with_segment = mesh.signed_distance_grid(v2, t2, lo, hi, ws)
    plain = mesh.signed_distance_grid(bv, bt, lo, hi, ws)
    assert torch.equal(with_segment < 0, plain < 0) and int((plain < 0).sum()) > 20
    n2 = R.grid_nodes(lo, hi, ws)
    want2 = R.unsigned_distance(n2, v2, t2)[0]
    assert np.abs(with_segment.abs().cpu().numpy().reshape(-1) - want2).max() <= R.tolerance(n2, v2, t2, want2)[0]
    assert bool((with_segment.abs() < plain.abs()).any())                           # and it takes part in the distance


# ---- 5. self-consistency ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['sphere', 'torus', 'box'])
def test_closest_point_lies_on_the_returned_triangle_at_the_returned_distance(name):
    from poseprobe_amd import mesh
    c = case(name)
    d, closest, tri = mesh.unsigned_distance(c['nodes'], c['v'], c['t'])
    assert d.dtype == torch.float32 and closest.dtype == torch.float32 and tri.dtype == torch.int32 and d.is_cuda
    assert tuple(closest.shape) == (len(c['nodes']), 3)
    assert np.abs(d.cpu().numpy() - np.abs(c['ref'])).max() <= c['tol']
    check_self_consistent(c['nodes'], c['v'], c['t'], d, closest, tri, c['tol'])
    grid = mesh.signed_distance_grid(c['v'], c['t'], *c['grid'])
    assert torch.equal(grid.abs().reshape(-1), d)                                   # the nodes of the grid are these very queries


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_open_meshes_nan_vertices_and_bad_indices_are_refused():
    from poseprobe_amd import mesh
    c = case('box')
    v, t = c['v'], c['t']
    with pytest.raises(ValueError, match='3 edges'):
        mesh.signed_distance_grid(v, t[1:], *c['grid'])
    with pytest.raises(ValueError, match='3 edges'):
        mesh.signed_distance_grid(dev(v), dev(t[1:]), *c['grid'])
    bad = np.array(v)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match='non-finite'):
        mesh.signed_distance_grid(bad, t, *c['grid'])
    far = np.array(t)
    far[5, 2] = len(v)
    with pytest.raises(ValueError, match='index'):
        mesh.signed_distance_grid(v, far, *c['grid'])
    with pytest.raises(ValueError, match='index'):
        mesh.signed_distance_grid(dev(v), dev(far), *c['grid'])
    with pytest.raises(ValueError, match='index'):
        mesh.unsigned_distance(c['nodes'], v, far)
    # the distance needs no closed mesh
    d, closest, tri = mesh.unsigned_distance(c['nodes'], v, t[1:])
    want = R.unsigned_distance(c['nodes'], v, t[1:])[0]
    assert np.abs(d.cpu().numpy() - want).max() <= c['tol']
    # and check=False leaves the parity of an open mesh to the caller: no refusal, same magnitudes
    g = mesh.signed_distance_grid(v, t[1:], *c['grid'], check=False)
    assert torch.equal(g.abs().reshape(-1), d)


# ---- 7. bit-reproducibility ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['nested', 'box'])
def test_two_calls_return_equal_bits(name):
    from poseprobe_amd import mesh
    c = case(name)
    v, t, q = dev(c['v']), dev(c['t']), dev(c['nodes'])
    a, b = (mesh.signed_distance_grid(v, t, *c['grid']) for _ in range(2))
    assert torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))
    first, second = (mesh.unsigned_distance(q, v, t) for _ in range(2))
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    assert torch.equal(a, mesh.signed_distance_grid(c['v'], c['t'], *c['grid']))    # numpy in, the same bits out


# ---- 8. inverse of marching cubes, and the plumbing up to a train step -------------------------------------------------------------------
G = 24


def probe_model():
    from tests.test_mesh_sdf_host import _model
    return _model(G).cuda()


@functools.lru_cache(maxsize=None)
def probe_mesh():
    return frozen(*R.sphere(3, 0.25, (0.0, 0.0, -0.1)))


def test_template_from_mesh_is_the_inverse_of_marching_cubes():
    from poseprobe_amd import mesh
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    v, t = probe_mesh()
    model = probe_model()
    assert model.world_size.tolist() == [G] * 3
    cube = model.sdf.grid.detach().clone()
    sdf = mesh.voxurf_template_from_mesh(model, v, t)
    assert tuple(sdf.shape) == (G, G, G) and sdf.is_cuda and not torch.equal(model.sdf.grid.detach(), cube)
    assert torch.equal(sdf, mesh.signed_distance_grid(v, t, syn.XYZ_MIN, syn.XYZ_MAX, (G, G, G)))
    assert torch.equal(model.sdf.grid.detach()[0, 0], sdf) and not model.sdf.grid.requires_grad
    eng = TrainEngine(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(syn.range_shape().max())), 3, 24, 24, 96, device='cuda:0')
    eng.set_template(sdf)
    assert torch.equal(eng.sdf, sdf)
    eng.set_template(model.sdf.grid.detach().cpu())                                 # [1,1,X,Y,Z], from the host
    assert torch.equal(eng.sdf, sdf)
    with pytest.raises(ValueError):
        eng.set_template(sdf[:-1])
    # against the analytic sphere: within the Hausdorff distance of the polyhedron
    nodes = R.grid_nodes(syn.XYZ_MIN, syn.XYZ_MAX, (G, G, G)).astype(np.float64)
    want = np.linalg.norm(nodes - np.array([[0.0, 0.0, -0.1]]), axis=1) - 0.25
    slack = 0.25 - R.smallest_face_distance(v, t, (0.0, 0.0, -0.1)) + 1e-6
    assert np.abs(sdf.cpu().numpy().reshape(-1) - want).max() <= slack
    # extract on the node lattice: every vertex lies on a lattice edge the mesh crosses, so within one voxel edge of the mesh
    h = float(syn.XYZ_MAX[0] - syn.XYZ_MIN[0]) / (G - 1)
    ev, et = mesh.voxurf_extract_geometry(model, syn.XYZ_MIN, syn.XYZ_MAX, resolution=G)
    assert len(ev) > 100 and len(et) > 200
    d, _, _ = mesh.unsigned_distance(ev.astype(np.float32), v, t)
    print(f'extracted {len(ev)} vertices, {len(et)} triangles; farthest from the input mesh {float(d.max()):.4g}, voxel edge {h:.4g}')
    assert float(d.max()) <= h * (1 + 1e-4)
    edges = np.sort(np.concatenate([et[:, [0, 1]], et[:, [1, 2]], et[:, [2, 0]]]), axis=1)
    uniq, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()                                                      # closed, a manifold
    assert len(np.unique(et)) - len(uniq) + len(et) == 2                            # Euler characteristic of a sphere


def test_one_train_step_runs_on_a_mesh_template():
    from oracle import voxurf_oracle as O
    from poseprobe_amd import mesh
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    H = W = 24
    N, V = 96, 3
    rs = syn.range_shape()
    views = syn.make_views(V, H, W)
    idx, jit = syn.step_randomness(V * H * W, N, seed=1)
    scene = O.Scene(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, output_range=float(rs.max()), rect_size=rs.tolist())
    P = O.init_params(scene, seed=2)
    eng = TrainEngine(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max())), V, H, W, N, device='cuda:0')
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    v, t = probe_mesh()
    sdf = mesh.signed_distance_grid(v, t, syn.XYZ_MIN, syn.XYZ_MAX, eng.sdf.shape)
    eng.set_template(sdf)
    k0_before = eng.k0_cl.clone()
    eng.zero_grads()
    eng.train_step(torch.tensor(idx, dtype=torch.int32, device='cuda:0'), torch.tensor(jit, device='cuda:0'), 10)
    torch.cuda.synchronize()
    M = int(eng.ws.count.item())
    print(f'{M} samples marched on the sphere template')
    assert M > 0 and torch.equal(eng.sdf, sdf)                                      # the template stays frozen
    assert bool(torch.isfinite(eng.ws.rgb_marched).all()) and bool(torch.isfinite(eng.k0_cl).all())
    assert bool(torch.isfinite(eng.flat.data).all()) and bool(torch.isfinite(eng.se3).all())
    assert not torch.equal(eng.k0_cl, k0_before)                                    # the step did train
