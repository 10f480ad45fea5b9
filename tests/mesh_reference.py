"""Numpy restatement of the marching-cubes semantics of include/poseprobe_hip.h (pp_mc_*), used as the reference of the GPU
tests, plus the test fields and the mesh checks shared by tests/test_mesh_host.py and tests/test_hip_mesh.py.

It shares only the 256-case table with the kernels (pp_mc_table, whose properties test_mesh_host.py checks exhaustively); it is
itself checked against mathematics (closed manifolds, Euler characteristics, interpolation error and volume bounds of a sphere),
not against the code under test.

  corner below  <=>  u < threshold (fp32);  edge active  <=>  exactly one endpoint below, owned by its lower endpoint p0 and axis a
  vertex: t = (threshold - u[p0]) / (u[p1] - u[p0]) in fp32, coordinate a = float(p0[a]) + t
  vertex id = rank of the edge among the active edges in the order 3 * (x Y Z + y Z + z) + a
  triangles ordered by cell (C order over (X-1, Y-1, Z-1)), then by table row order
"""
import functools

import numpy as np

CORNER = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])


def edge_p0(e):
    """Offset of the lower endpoint of cube edge e (axis a = e >> 2) from the cell's low corner."""
    a, j = e >> 2, e & 3
    p = [0, 0, 0]
    b, c = [k for k in range(3) if k != a]
    p[b], p[c] = j & 1, j >> 1
    return p


EDGE_P0 = np.array([edge_p0(e) for e in range(12)])
EDGE_AXIS = np.arange(12) >> 2


@functools.lru_cache(maxsize=None)
def table():
    from poseprobe_amd import ops
    t = ops.mc_table()
    t.setflags(write=False)
    return t


def case_index(u, threshold):
    """[X-1,Y-1,Z-1] case index of every cell."""
    below = np.asarray(u, dtype=np.float32) < np.float32(threshold)
    X, Y, Z = below.shape
    case = np.zeros((X - 1, Y - 1, Z - 1), dtype=np.int32)
    for c, (dx, dy, dz) in enumerate(CORNER):
        case |= below[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz].astype(np.int32) << c
    return case


def marching_cubes(u, threshold):
    """u [X,Y,Z] -> (vertices [Nv,3] float32 in lattice coordinates, triangles [Nt,3] int32)."""
    u = np.ascontiguousarray(u, dtype=np.float32)
    thr = np.float32(threshold)
    X, Y, Z = u.shape
    below = u < thr
    active = np.zeros((X, Y, Z, 3), dtype=bool)
    active[:-1, :, :, 0] = below[:-1] != below[1:]
    active[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    active[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    flat = active.reshape(-1)
    vid = (np.cumsum(flat, dtype=np.int64) - 1).reshape(X, Y, Z, 3)          # valid where active
    where = np.flatnonzero(flat)
    lin, axis = where // 3, where % 3
    stride = np.array([Y * Z, Z, 1])
    u0, u1 = u.reshape(-1)[lin], u.reshape(-1)[lin + stride[axis]]
    with np.errstate(all='ignore'):
        t = (thr - u0) / (u1 - u0)                                             # float32 throughout
    assert t.dtype == np.float32
    vertices = np.stack(np.unravel_index(lin, (X, Y, Z)), axis=-1).astype(np.float32)
    vertices[np.arange(len(lin)), axis] += t
    case = case_index(u, thr)
    tab = table()
    ntri = (tab[:, ::3] >= 0).sum(axis=1)
    cell = np.flatnonzero(ntri[case.reshape(-1)] > 0)
    cx, cy, cz = np.unravel_index(cell, case.shape)
    ccase = case.reshape(-1)[cell]
    keys, tris = [], []
    for k in range(5):
        sel = ntri[ccase] > k
        e = tab[ccase[sel], 3 * k:3 * k + 3]                                   # [n,3] edge ids
        p0 = EDGE_P0[e]                                                       # [n,3,3]
        ids = vid[cx[sel, None] + p0[..., 0], cy[sel, None] + p0[..., 1], cz[sel, None] + p0[..., 2], EDGE_AXIS[e]]
        assert active[cx[sel, None] + p0[..., 0], cy[sel, None] + p0[..., 1], cz[sel, None] + p0[..., 2], EDGE_AXIS[e]].all()
        tris.append(ids)
        keys.append(cell[sel] * 5 + k)
    keys, tris = np.concatenate(keys), np.concatenate(tris)
    triangles = tris[np.argsort(keys, kind='stable')].astype(np.int32).reshape(-1, 3)
    return vertices.reshape(-1, 3), triangles


# ---- mesh checks ------------------------------------------------------------------------------------------------------------
def directed_sides(triangles):
    t = np.asarray(triangles, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def is_closed_manifold(triangles, n_vertices):
    """Every directed side occurs once and its reverse occurs once."""
    s = directed_sides(triangles)
    key, rev = s[:, 0] * n_vertices + s[:, 1], s[:, 1] * n_vertices + s[:, 0]
    return len(np.unique(key)) == len(key) and np.array_equal(np.sort(key), np.sort(rev))


def euler_characteristic(triangles, n_vertices):
    s = np.sort(directed_sides(triangles), axis=1)
    edges = len(np.unique(s[:, 0] * n_vertices + s[:, 1]))
    return n_vertices - edges + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(triangles)[:, k]] for k in range(3))
    return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


# ---- test fields ------------------------------------------------------------------------------------------------------------
def lattice_points(shape):
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij'), axis=-1)


SPHERE = dict(shape=(25, 21, 23), c=np.array([12.3, 10.1, 11.4]), r=8.37)
TORUS = dict(shape=(25, 21, 23), c=np.array([12.2, 10.3, 11.1]), R=6.3, tube=2.4)


def sphere_field(shape=SPHERE['shape'], c=SPHERE['c'], r=SPHERE['r']):
    """u = r - |x - c|: positive inside."""
    return (r - np.linalg.norm(lattice_points(shape) - c, axis=-1)).astype(np.float32)


def torus_field(shape=TORUS['shape'], c=TORUS['c'], R=TORUS['R'], tube=TORUS['tube']):
    d = lattice_points(shape) - c
    return (tube - np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - R) ** 2 + d[..., 2] ** 2)).astype(np.float32)


def noise_field(shape, seed=0, closed=False):
    u = np.random.RandomState(seed).randn(*shape).astype(np.float32)
    if closed:                                   # the six boundary layers below the threshold 0: the surface cannot leave the lattice
        u[0], u[-1], u[:, 0], u[:, -1], u[:, :, 0], u[:, :, -1] = (-1.0,) * 6
    return u


def plane_field(shape=(8, 6, 5)):
    """u = x - 3: lattice values exactly at the threshold 0."""
    return np.broadcast_to(np.arange(shape[0], dtype=np.float32)[:, None, None] - 3.0, shape).copy()


def big_field():
    """Odd sizes and 600 of the kernels' 1024-point tiles (an x step is 4690 points, a y step 70): a sphere plus low-amplitude
    noise, whose surface crosses tile borders along every axis."""
    shape = (131, 67, 70)
    u = sphere_field(shape, np.array([64.2, 33.1, 35.7]), 27.3)
    return u + 0.3 * np.random.RandomState(1).randn(*shape).astype(np.float32)


def sphere_checks(vertices, triangles, c=SPHERE['c'], r=SPHERE['r'], h=1.0):
    """The properties a marching-cubes mesh of the sphere field must have (tests/test_mesh_host.py states their origin)."""
    v = np.asarray(vertices, dtype=np.float64)
    assert is_closed_manifold(triangles, len(v))
    assert euler_characteristic(triangles, len(v)) == 2
    dev = np.abs(np.linalg.norm(v - c, axis=1) - r).max()
    bound = h * h / (8 * (r - h)) + 1e-4
    assert dev <= bound, (dev, bound)
    vol = signed_volume(v, triangles)
    lo = 4 / 3 * np.pi * (r - 3 * h * h / (8 * r) - h * h / (8 * (r - h))) ** 3
    hi = 4 / 3 * np.pi * (r + h * h / (8 * (r - h))) ** 3
    assert 0 < lo <= vol <= hi, (lo, vol, hi)
    return dev, bound, vol, lo, hi
