"""Numpy reference of mesh -> signed distance (poseprobe_amd.mesh.unsigned_distance / signed_distance_grid): the
yardstick the GPU tests compare with.  It shares nothing with the kernels: no cell grid (every triangle is tried for every
query), the closest point by the region tests of Ericson's "Real-Time Collision Detection" §5.1.5 (the kernels take the best of
the perpendicular's foot and three segments), and the sign by the parity of the Moeller-Trumbore hits of ONE ray per node in a
generic direction (the kernels count the crossings of axis-parallel columns under a fill rule).  float64 by default; `dtype=
np.float32` restates the distance routine in float32, and the deviation between the two sets the tolerance of the comparison.
tests/test_mesh_sdf_host.py checks this file against mathematics: boxes, spheres, hollow spheres."""
import numpy as np

from tests.dtu_eval_reference import icosphere

RAY = np.array([2.0 ** 0.5 - 1.0, 3.0 ** 0.5 - 1.0, 5.0 ** 0.5 / 3.0])      # pairwise irrational ratios: parallel to no face of the cases
RAY = RAY / np.linalg.norm(RAY)


# ---------------------------------------------------------------------------------------------------------------------- meshes
def sphere(level, radius, centre, reverse=False):
    v, t = icosphere(level)
    v = v * radius + np.asarray(centre, np.float64)[None]
    return v.astype(np.float32), np.ascontiguousarray(t[:, ::-1] if reverse else t).astype(np.int32)


def nested_spheres(level, r_outer, r_inner, centre):
    """An outer sphere and an inner one with reversed winding: a shell, whose cavity is outside."""
    vo, to = sphere(level, r_outer, centre)
    vi, ti = sphere(level, r_inner, centre, reverse=True)
    return np.concatenate([vo, vi]), np.concatenate([to, ti + len(vo)]).astype(np.int32)


def torus(nu, nv, R, r, centre):
    """nu x nv quads around the z axis through `centre`, each split into two triangles."""
    u, w = np.meshgrid(np.arange(nu) * (2 * np.pi / nu), np.arange(nv) * (2 * np.pi / nv), indexing='ij')
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], -1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)
    t = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            t += [(a, b, c), (a, c, d)]
    return (v + np.asarray(centre, np.float64)[None]).astype(np.float32), np.array(t, np.int32)


def box(lo, hi):
    """The axis-aligned box as 8 vertices and 12 triangles, outward winding."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])          # bit a of the index: low or high along a
    q = [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]  # -x +x -y +y -z +z
    t = [f for a, b, c, d in q for f in ((a, b, c), (a, c, d))]
    return v.astype(np.float32), np.array(t, np.int32)


def tetrahedron(centre, size):
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * size + np.asarray(centre, np.float64)[None]
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)


def grid_axes(xyz_min, xyz_max, world_size):
    """Node coordinates: float64, rounded once to float32 - the nodes both the reference and the kernels see."""
    return [(np.float64(lo) + np.arange(n, dtype=np.float64) * ((np.float64(hi) - np.float64(lo)) / (n - 1))).astype(np.float32)
            for lo, hi, n in zip(xyz_min, xyz_max, world_size)]


def grid_nodes(xyz_min, xyz_max, world_size):
    """[X*Y*Z,3] float32, x-major."""
    return np.stack(np.meshgrid(*grid_axes(xyz_min, xyz_max, world_size), indexing='ij'), -1).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------- distance
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _safe_div(n, d):
    return np.divide(n, d, out=np.zeros_like(n), where=d != 0)


def _closest_on_segments(p, a, b):
    ab = b - a
    num = _dot(p - a, ab)
    s = np.clip(_safe_div(num, np.broadcast_to(_dot(ab, ab), num.shape)), 0, 1)
    return a + s[..., None] * ab


def closest_on_triangles(p, a, b, c):
    """p [Q,1,3], a, b, c [1,T,3] -> the closest point [Q,T,3] of every triangle to every query.  Ericson's regions for a triangle
    with area; a triangle without area is the nearest of its three sides taken as segments (a side without length is a point)."""
    ab, ac, ap = b - a, c - a, p - a
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = p - b
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = p - c
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one = np.ones_like(d1)
    zero = np.zeros_like(d1)
    den = _safe_div(one, va + vb + vc)
    v, w = vb * den, vc * den                                                  # interior
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    e_bc = _safe_div(d4 - d3, (d4 - d3) + (d5 - d6))
    vs = [zero, one, _safe_div(d1, d1 - d3), zero, zero, 1 - e_bc]
    ws = [zero, zero, zero, one, _safe_div(d2, d2 - d6), e_bc]
    v, w = np.select(conds, vs, v), np.select(conds, ws, w)
    out = a + v[..., None] * ab + w[..., None] * ac
    n = np.cross(ab, ac)
    flat = (_dot(n, n) == 0)[0]                                                # [T]
    if flat.any():
        af, bf, cf = a[:, flat], b[:, flat], c[:, flat]
        cand = np.stack([_closest_on_segments(p, af, bf), _closest_on_segments(p, bf, cf), _closest_on_segments(p, cf, af)])
        d = ((cand - p[None]) ** 2).sum(-1)
        pick = d.argmin(0)
        out[:, flat] = np.take_along_axis(cand, pick[None, ..., None], 0)[0]
    return out


def unsigned_distance(points, vertices, triangles, dtype=np.float64, chunk=256):
    """Brute force: -> (dist [Q], closest [Q,3], triangle [Q]) in `dtype`; ties go to the lowest triangle (argmin's first)."""
    p, v = np.asarray(points).astype(dtype), np.asarray(vertices).astype(dtype)
    t = np.asarray(triangles)
    a, b, c = v[t[:, 0]][None], v[t[:, 1]][None], v[t[:, 2]][None]
    dist, closest, tri = np.empty(len(p), dtype), np.empty((len(p), 3), dtype), np.empty(len(p), np.int32)
    for s in range(0, len(p), chunk):
        q = p[s:s + chunk, None]
        cl = closest_on_triangles(q, a, b, c)
        d = cl - q
        d2 = _dot(d, d)
        i = d2.argmin(1)
        r = np.arange(len(i))
        dist[s:s + chunk], closest[s:s + chunk], tri[s:s + chunk] = np.sqrt(d2[r, i]), cl[r, i], i
    return dist, closest, tri


# ---------------------------------------------------------------------------------------------------------------------- sign
def inside(points, vertices, triangles, direction=RAY, chunk=256):
    """bool [Q]: odd number of Moeller-Trumbore hits (t > 0) of the ray from each point along `direction`; float64.  A triangle
    parallel to the ray is missed, as one without area is."""
    p, v = np.asarray(points, np.float64), np.asarray(vertices, np.float64)
    t = np.asarray(triangles)
    a, e1, e2 = v[t[:, 0]][None], (v[t[:, 1]] - v[t[:, 0]])[None], (v[t[:, 2]] - v[t[:, 0]])[None]
    d = np.asarray(direction, np.float64)[None, None]
    h = np.cross(d, e2)
    det = _dot(e1, h)
    ok = det != 0
    inv = _safe_div(np.ones_like(det), det)
    out = np.empty(len(p), bool)
    for s in range(0, len(p), chunk):
        sv = p[s:s + chunk, None] - a
        u = _dot(sv, h) * inv
        q = np.cross(sv, e1)
        w = _dot(d, q) * inv
        tt = _dot(e2, q) * inv
        hit = ok & (u >= 0) & (w >= 0) & (u + w <= 1) & (tt > 0)
        out[s:s + chunk] = hit.sum(1) % 2 == 1
    return out


def signed_distance(points, vertices, triangles):
    """float64 [Q], negative inside."""
    d = unsigned_distance(points, vertices, triangles)[0]
    return np.where(inside(points, vertices, triangles), -d, d)


def odd_edges(triangles):
    """Undirected edges with an odd number of incident triangles."""
    count = {}
    for tri in np.asarray(triangles).tolist():
        for i in range(3):
            a, b = tri[i], tri[(i + 1) % 3]
            if a != b:
                count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
    return sum(1 for c in count.values() if c % 2)


# ---------------------------------------------------------------------------------------------------------------------- tolerance
def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def tolerance(points, vertices, triangles, d64=None):
    """(tolerance, deviation): 4 x the largest deviation of the float32 restatement of unsigned_distance from float64 on this very
    case, and no less than 4 float32 ulps of the largest coordinate magnitude in play."""
    if d64 is None:
        d64 = unsigned_distance(points, vertices, triangles)[0]
    d32 = unsigned_distance(points, vertices, triangles, dtype=np.float32)[0]
    dev = float(np.abs(d32.astype(np.float64) - d64).max())
    big = max(float(np.abs(np.asarray(points, np.float64)).max()), float(np.abs(np.asarray(vertices, np.float64)).max()))
    return max(4 * dev, 4 * ulp32(big)), dev


# ---------------------------------------------------------------------------------------------------------------------- analytic
def box_sdf(points, lo, hi):
    p, lo, hi = np.asarray(points, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    q = np.abs(p - (lo + hi) / 2) - (hi - lo) / 2
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)


def smallest_face_distance(vertices, triangles, centre):
    """rho: the smallest distance of a face's plane from the centre (float64).  For a polyhedron inscribed in the sphere of radius r
    about the centre, r - rho is the Hausdorff distance between the two surfaces."""
    v = np.asarray(vertices, np.float64) - np.asarray(centre, np.float64)[None]
    t = np.asarray(triangles)
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    return float(np.abs(_dot(n, v[t[:, 0]]) / np.linalg.norm(n, axis=1)).min())


def init_sdf_from_sdf(sdf0, world_size, smooth=False, reduce=1., ksize=3, sigma=1.):
    """float64 restatement of the three steps of lib/voxurf_coarse.py:287-299 on sdf0 [X0,Y0,Z0] -> [X,Y,Z]: the trilinear
    align_corners=True resize (when the shapes differ), the Gaussian with replicate padding over sdf0 / reduce, and the division by
    `reduce` - which the smooth branch therefore applies twice."""
    g = np.asarray(sdf0, np.float64)
    if tuple(g.shape) != tuple(world_size):
        for ax, n in enumerate(world_size):
            m = g.shape[ax]
            x = np.arange(n, dtype=np.float64) * ((m - 1) / (n - 1) if n > 1 else 0.0)
            i0 = np.minimum(np.floor(x).astype(int), max(m - 2, 0))
            f = x - i0
            i1 = np.minimum(i0 + 1, m - 1)
            shape = [1, 1, 1]
            shape[ax] = n
            g = np.take(g, i0, ax) * (1 - f).reshape(shape) + np.take(g, i1, ax) * f.reshape(shape)
    if not smooth:
        return g / reduce
    h = ksize // 2
    r = np.arange(-h, h + 1)
    xx, yy, zz = np.meshgrid(r, r, r, indexing='ij')
    k = np.exp(-(xx ** 2 + yy ** 2 + zz ** 2) / (2 * sigma ** 2))
    k = k / k.sum()
    pad = np.pad(g / reduce, h, mode='edge')
    out = np.zeros_like(g)
    for i in range(ksize):
        for j in range(ksize):
            for l in range(ksize):
                out += k[i, j, l] * pad[i:i + g.shape[0], j:j + g.shape[1], l:l + g.shape[2]]
    return out / reduce
