"""Numpy restatement of the connected-component semantics of include/poseprobe_hip.h (pp_cc_*) and of
poseprobe_amd.mesh.connected_components / keep_components, used as the reference of tests/test_hip_mesh_components.py, plus the
meshes those tests and tests/test_mesh_components_host.py share.

  two vertices are connected  <=>  some triangle contains both (a shared vertex is enough)
  labels[v] = the smallest vertex index of v's component, -1 for a vertex no triangle references
  roots = the labels that occur, ascending; a triangle belongs to the component of its vertices

`labels` is a plain union-find (a Python loop, no rounds): it shares nothing with the kernels.  test_mesh_components_host.py checks
it against scipy.sparse.csgraph.connected_components.  `rounds` restates the SCHEDULE of the kernels - hook on a snapshot, a jump of
HOPS further hops - which makes the number of rounds a pure function of the mesh; it is checked against `labels` on the host.
"""
import functools

import numpy as np

from tests import mesh_reference as M

HOPS = 2                     # csrc/pp_mesh_components.hip, CC_HOPS


def _find(parent, v):
    r = v
    while parent[r] != r:
        r = parent[r]
    while parent[v] != r:
        parent[v], v = r, parent[v]
    return r


def labels(triangles, n_vertices):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    parent = list(range(n_vertices))
    for a, b, c in t.tolist():
        for x, y in ((a, b), (a, c)):
            rx, ry = _find(parent, x), _find(parent, y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)           # the root of a set is its smallest member
    out = np.array([_find(parent, v) for v in range(n_vertices)], dtype=np.int32).reshape(n_vertices)
    referenced = np.zeros(n_vertices, dtype=bool)
    referenced[t.reshape(-1)] = True
    out[~referenced] = -1
    return out


def connected_components(triangles, n_vertices):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    lab = labels(t, n_vertices)
    roots = np.unique(lab[lab >= 0]).astype(np.int32)
    vertex_counts = np.array([(lab == r).sum() for r in roots], dtype=np.int32).reshape(len(roots))
    tri_label = lab[t[:, 0]] if len(t) else np.empty(0, np.int32)
    triangle_counts = np.array([(tri_label == r).sum() for r in roots], dtype=np.int32).reshape(len(roots))
    return dict(labels=lab, roots=roots, vertex_counts=vertex_counts, triangle_counts=triangle_counts, n_components=len(roots))


def kept_roots(cc, keep):
    """The roots `keep` selects: 'largest' (most triangles, ties to the lowest root), an int (minimum triangle count) or a float in
    (0, 1) (minimum fraction of the largest count, decided in float64 as count >= keep * largest)."""
    tc = cc['triangle_counts']
    if cc['n_components'] == 0:
        return cc['roots'][:0]
    if keep == 'largest':
        return cc['roots'][[int(np.flatnonzero(tc == tc.max())[0])]]
    if isinstance(keep, (int, np.integer)):
        return cc['roots'][tc >= keep]
    return cc['roots'][tc.astype(np.float64) >= np.float64(keep) * np.float64(tc.max())]


def keep_components(vertices, triangles, keep='largest', attributes=None):
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int32).reshape(-1, 3)
    cc = connected_components(t, len(v))
    roots = kept_roots(cc, keep)
    vkeep = np.isin(cc['labels'], roots) & (cc['labels'] >= 0)
    tkeep = vkeep[t[:, 0]] if len(t) else np.zeros(0, dtype=bool)
    index = np.flatnonzero(vkeep).astype(np.int32)
    new = np.full(len(v), -1, dtype=np.int32)
    new[index] = np.arange(len(index), dtype=np.int32)
    out = dict(vertices=v[index], triangles=new[t[tkeep]].reshape(-1, 3), vertex_index=index, n_components=cc['n_components'],
               n_kept=len(roots))
    assert (out['triangles'] >= 0).all()
    for k, a in (attributes or {}).items():
        out[k] = np.asarray(a)[index]
    return out


def rounds(triangles, n_vertices, hops=HOPS, limit=100000):
    """(labels, rounds) of the kernels' schedule: every round hooks on a snapshot L (P[label] <- min over the triangles' minima),
    then every vertex takes P^(hops)(P[v]); rounds counts up to and including the first round that changes nothing."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    L = np.full(n_vertices, -1, dtype=np.int64)
    L[t.reshape(-1)] = t.reshape(-1)
    if len(t) == 0:
        return L.astype(np.int32), 0
    ref = L >= 0
    for r in range(1, limit + 1):
        P = L.copy()
        lab = L[t]                                          # [Nt,3]
        m = lab.min(axis=1, keepdims=True)
        np.minimum.at(P, lab.reshape(-1), np.broadcast_to(m, lab.shape).reshape(-1))
        new = P.copy()
        for _ in range(hops):
            new[ref] = P[new[ref]]
        if np.array_equal(new, L):
            return L.astype(np.int32), r
        L = new
    raise AssertionError('no fixpoint')


# ---- meshes -----------------------------------------------------------------------------------------------------------------
def strip(n_triangles, numbering, seed=0):
    """A triangle strip (triangle i on positions i, i+1, i+2 of a row of n_triangles + 2 vertices) with the positions numbered
    ascending, descending or by a seeded random permutation -> (triangles [Nt,3] int32, n_vertices)."""
    nv = n_triangles + 2
    i = np.arange(n_triangles)
    t = np.stack([i, i + 1, i + 2], axis=-1)
    t[1::2] = t[1::2][:, [1, 0, 2]]                         # alternate the order so that the winding is consistent
    if numbering == 'ascending':
        number = np.arange(nv)
    elif numbering == 'descending':
        number = np.arange(nv)[::-1].copy()
    elif numbering == 'random':
        number = np.random.RandomState(seed).permutation(nv)
    else:
        raise ValueError(numbering)
    return number[t].astype(np.int32), nv


STRIP_TRIANGLES = 4096

SHAPE = (24, 24, 24)
SPHERE_A = dict(c=np.array([7.4, 7.6, 15.5]), r=4.2)
SPHERE_B = dict(c=np.array([17.1, 16.2, 16.3]), r=2.6)
TORUS = dict(c=np.array([11.6, 11.4, 5.2]), R=5.5, tube=2.0)
BIG = dict(c=np.array([9.3, 10.1, 11.4]), r=6.37)
SMALL = dict(c=np.array([19.2, 18.4, 18.7]), r=2.45)       # |c_big - c_small| - r_big - r_small = 6.6 cells


def three_body_field():
    """Two spheres of different radius and a torus, pairwise more than two cells apart: u = max of the three (positive inside)."""
    return np.maximum(np.maximum(M.sphere_field(SHAPE, **SPHERE_A), M.sphere_field(SHAPE, **SPHERE_B)), M.torus_field(SHAPE, **TORUS))


def noise_field():
    return M.noise_field(SHAPE, seed=3)


def big_field():
    return M.sphere_field(SHAPE, **BIG)


def big_and_small_field():
    """min(d_big, d_small) in distances = max in the positive-inside convention of the test fields."""
    return np.maximum(big_field(), M.sphere_field(SHAPE, **SMALL))


@functools.lru_cache(maxsize=None)
def mc_mesh(name):
    """(vertices, triangles) of the restated marching cubes (tests/mesh_reference.py) on one of the fields above, read-only."""
    v, t = M.marching_cubes(globals()[name + '_field'](), 0.0)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t


def component_mesh(cc, triangles, root):
    """(triangles renumbered to the component's own vertices, its vertex count)."""
    t = np.asarray(triangles)
    sel = cc['labels'][t[:, 0]] == root
    index = np.flatnonzero(cc['labels'] == root)
    new = np.full(len(cc['labels']), -1, dtype=np.int64)
    new[index] = np.arange(len(index))
    return new[t[sel]], len(index)


def small_cases():
    """name -> (triangles [Nt,3] int32, n_vertices): the hand-made cases of the index-by-index tests."""
    tri = lambda *rows: np.array(rows, dtype=np.int32).reshape(-1, 3)
    return {
        'no_triangle': (tri(), 5),
        'no_vertex': (tri(), 0),
        'one_triangle': (tri([0, 1, 2]), 3),
        'two_disjoint': (tri([0, 1, 2], [3, 4, 5]), 6),
        'shared_vertex': (tri([0, 1, 2], [2, 3, 4]), 5),
        'unreferenced': (tri([2, 3, 5], [5, 9, 8], [11, 12, 13], [6, 11, 6]), 16),      # 0 1 | 4 7 10 | 14 15 are in no triangle
    }
