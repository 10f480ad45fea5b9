"""Mesh extraction, the part that needs no GPU: the 256-case table's properties (exhaustively), the numpy restatement of the
marching-cubes semantics against mathematics (tests/mesh_reference.py - the reference the GPU tests compare with), argument
validation of the four pp_mc_* entry points, the PLY writer, and the legacy names, which keep refusing."""
import ctypes
import itertools
import struct

import numpy as np
import pytest
import torch

from tests import mesh_reference as R

EDGE_ENDS = [(tuple(R.EDGE_P0[e]), tuple(R.EDGE_P0[e] + np.eye(3, dtype=int)[e >> 2])) for e in range(12)]
MID = np.array([(np.array(a) + np.array(b)) / 2.0 for a, b in EDGE_ENDS])


def corner_id(p):
    return p[0] + 2 * p[1] + 4 * p[2]


def rows():
    return [[tuple(int(v) for v in row[3 * k:3 * k + 3]) for k in range(5) if row[3 * k] >= 0] for row in R.table()]


def sides_of(tris):
    return [s for a, b, c in tris for s in ((a, b), (b, c), (c, a))]


def on_face(e, axis, side):
    return all(p[axis] == side for p in EDGE_ENDS[e])


# ---- 1. table properties --------------------------------------------------------------------------------------------------------
def test_table_rows_are_well_formed():
    t = R.table()
    assert t.shape == (256, 16) and t.dtype == np.int32
    for case, row in enumerate(t):
        n = int((row >= 0).sum())
        assert n % 3 == 0 and n <= 15, case
        assert (row[:n] >= 0).all() and (row[:n] <= 11).all() and (row[n:] == -1).all(), case
        for k in range(n // 3):
            assert len(set(row[3 * k:3 * k + 3])) == 3, (case, k)
    assert (t[0] == -1).all() and (t[255] == -1).all()
    assert sum(len(r) for r in rows()) == int((t[:, ::3] >= 0).sum())


def test_table_uses_exactly_the_crossed_edges():
    for case, tris in enumerate(rows()):
        crossed = {e for e, (a, b) in enumerate(EDGE_ENDS) if ((case >> corner_id(a)) ^ (case >> corner_id(b))) & 1}
        assert {e for t in tris for e in t} == crossed, case


def test_table_sides_pair_up_inside_and_lie_on_faces_outside():
    for case, tris in enumerate(rows()):
        sides = sides_of(tris)
        assert len(set(sides)) == len(sides), f'case {case}: a directed side occurs twice'
        for a, b in sides:
            shared = any(on_face(a, ax, s) and on_face(b, ax, s) for ax in range(3) for s in range(2))
            if (b, a) not in sides:             # boundary side: both of its edges on one common cube face
                assert shared, (case, a, b)
            else:                               # interior side: strictly inside the cell - inside a face it could coincide with
                assert not shared, (case, a, b)  # a side of the cell beyond that face and belong to more than two triangles


def face_local(e, axis):
    """Name of cube edge e within a face normal to `axis`: (which of the face's two axes it runs along, its position 0 / 1)."""
    b, c = [k for k in range(3) if k != axis]
    run = e >> 2
    other = c if run == b else b
    return (0 if run == b else 1, EDGE_ENDS[e][0][other])


def face_function(axis, side):
    """{face bits: set of directed boundary sides in face-local names} over all 256 cases; asserts it is single-valued."""
    b, c = [k for k in range(3) if k != axis]
    out = {}
    for case, tris in enumerate(rows()):
        bits = 0
        for lb, lc in itertools.product(range(2), range(2)):
            p = [0, 0, 0]
            p[axis], p[b], p[c] = side, lb, lc
            bits |= ((case >> corner_id(p)) & 1) << (lb + 2 * lc)
        sides = sides_of(tris)
        here = frozenset((face_local(x, axis), face_local(y, axis)) for x, y in sides
                         if (y, x) not in sides and on_face(x, axis, side) and on_face(y, axis, side))
        assert out.setdefault(bits, here) == here, f'axis {axis} side {side}: face bits {bits:04b} give different sides in case {case}'
    assert len(out) == 16
    return out


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_table_faces_depend_on_their_corners_alone_and_match_across_cells(axis):
    low, high = face_function(axis, 0), face_function(axis, 1)
    for bits in range(16):
        # the cell below sees the shared face as its high face, the cell above as its low face: same segments, opposite direction
        assert frozenset((y, x) for x, y in high[bits]) == low[bits], (axis, bits)
        crossings = sum(((bits >> i) ^ (bits >> j)) & 1 for i, j in ((0, 1), (2, 3), (0, 2), (1, 3)))
        assert len(low[bits]) == crossings // 2


def test_table_single_corner_normals_point_below():
    tab = rows()
    for c in range(8):
        k = R.CORNER[c].astype(float)
        for case, sign in ((1 << c, 1.0), (255 ^ (1 << c), -1.0)):     # corner c alone below / alone above
            assert len(tab[case]) == 1
            v0, v1, v2 = (MID[e] for e in tab[case][0])
            assert sign * np.dot(np.cross(v1 - v0, v2 - v0), k - v0) > 0, case


# ---- 2. the numpy restatement against mathematics -----------------------------------------------------------------------------------
def test_reference_sphere():
    """Closed, genus 0, every vertex within the linear-interpolation error of a function with |f''| <= 1 / (r - h) along an edge
    (h^2 / (8 (r - h)), + 1e-4 for fp32), volume between the spheres of radius r - sagitta - that error and r + that error.
    With the generated table: 1322 vertices, 2640 triangles."""
    v, t = R.marching_cubes(R.sphere_field(), 0.0)
    assert v.dtype == np.float32 and t.dtype == np.int32 and v.shape[1] == 3 and t.shape[1] == 3
    dev, bound, vol, lo, hi = R.sphere_checks(v, t)
    print(f'sphere: {len(v)} vertices, {len(t)} triangles, deviation {dev:.4f} (bound {bound:.4f}), volume {vol:.1f} in [{lo:.1f}, {hi:.1f}]')


def test_reference_torus():
    v, t = R.marching_cubes(R.torus_field(), 0.0)
    assert len(t) > 0 and R.is_closed_manifold(t, len(v))
    assert R.euler_characteristic(t, len(v)) == 0


def test_reference_white_noise():
    v, t = R.marching_cubes(R.noise_field((14, 13, 12), closed=True), 0.0)
    assert len(t) > 0 and t.min() >= 0 and t.max() < len(v) and len(np.unique(t)) == len(v)
    assert R.is_closed_manifold(t, len(v))
    u = R.noise_field((20, 20, 20), seed=0)
    assert len(np.unique(R.case_index(u, 0.0))) == 256
    v, t = R.marching_cubes(u, 0.0)
    assert t.min() >= 0 and t.max() < len(v) and np.isfinite(v).all()


def test_reference_plane_and_empty_fields():
    v, t = R.marching_cubes(R.plane_field(), 0.0)
    assert np.isfinite(v).all() and (v[:, 0] == 3.0).all() and len(v) == 6 * 5 and len(t) == 40
    n = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    assert (n[:, 0] < 0).all() and (n[:, 1:] == 0).all()             # toward decreasing u
    for fill in (1.0, -1.0):
        v, t = R.marching_cubes(np.full((4, 3, 5), fill, np.float32), 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)


def test_reference_vertex_order_and_threshold():
    """Ids follow 3 * linear(p0) + axis; a non-zero threshold on a positive field."""
    u = np.full((2, 2, 2), 1.0, np.float32)
    u[0, 0, 0] = 0.0
    v, t = R.marching_cubes(u, 0.25)
    assert np.array_equal(v, np.array([[0.25, 0, 0], [0, 0.25, 0], [0, 0, 0.25]], np.float32))
    assert np.array_equal(t, np.array([R.table()[1, :3] // 4], np.int32))    # edges 0, 4, 8 carry vertices 0, 1, 2


# ---- 3. argument validation (before any GPU call) --------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)         # never dereferenced: every call below is refused first
LIMIT_OK, LIMIT_OVER = (2, 2, 178956970), (2, 2, 178956971)       # 3 X Y Z = 2^31 - 8 and 2^31 + 4


def _refused(rc, name, code=-1):
    from poseprobe_amd import _lib
    assert rc == code, (name, rc)
    assert name.encode() in _lib.lib().pp_last_error()


def test_mc_host_entry_points_validate():
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    _refused(L.pp_mc_table(None), 'pp_mc_table')
    b = ctypes.c_int64(-1)
    _refused(L.pp_mc_workspace(3, 3, 3, None), 'pp_mc_workspace')
    for dims in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (0, 3, 3), (-4, 3, 3)):
        _refused(L.pp_mc_workspace(*dims, ctypes.byref(b)), 'pp_mc_workspace')
    _refused(L.pp_mc_workspace(*LIMIT_OVER, ctypes.byref(b)), 'pp_mc_workspace', -3)
    _refused(L.pp_mc_workspace(1024, 1024, 1024, ctypes.byref(b)), 'pp_mc_workspace', -3)
    assert b.value == -1
    assert L.pp_mc_workspace(*LIMIT_OK, ctypes.byref(b)) == 0 and b.value >= 5 * 4 * 178956970
    n = 5 * 4 * 3
    assert 5 * n <= ops.mc_workspace(5, 4, 3) <= 5 * 1024 + 3 * 256
    with pytest.raises(_lib.PoseProbeError, match='at least 2'):
        ops.mc_workspace(5, 1, 3)


@pytest.mark.parametrize('entry', ['pp_mc_count', 'pp_mc_emit'])
def test_mc_device_entry_points_validate_before_any_gpu_call(entry):
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    X, Y, Z = 5, 4, 3
    need = ops.mc_workspace(X, Y, Z)

    def call(u=FAKE, dims=(X, Y, Z), work=FAKE, work_bytes=need, out=(FAKE, 7, FAKE, 9)):
        if entry == 'pp_mc_count':
            return L.pp_mc_count(u, *dims, 0.0, work, work_bytes, out[0], None)
        return L.pp_mc_emit(u, *dims, 0.0, work, work_bytes, *out, None)

    _refused(call(u=None), entry)
    _refused(call(work=None), entry)
    _refused(call(out=(None, 7, FAKE, 9)), entry)
    if entry == 'pp_mc_emit':
        _refused(call(out=(FAKE, 7, None, 9)), entry)
        _refused(call(out=(FAKE, -1, FAKE, 9)), entry)
        _refused(call(out=(FAKE, 7, FAKE, -1)), entry)
    for dims in ((1, Y, Z), (X, 1, Z), (X, Y, 1)):
        _refused(call(dims=dims), entry)
    _refused(call(dims=LIMIT_OVER, work_bytes=1 << 40), entry, -3)
    _refused(call(work_bytes=need - 1), entry)
    assert b'workspace' in L.pp_last_error()
    _refused(call(work=ctypes.c_void_p(4100)), entry)                # not 16-byte aligned


def test_marching_cubes_refuses_cpu_tensors():
    from poseprobe_amd import mesh
    with pytest.raises(RuntimeError, match='CUDA'):
        mesh.marching_cubes(torch.zeros(3, 3, 3), 0.0)
    with pytest.raises(TypeError):
        mesh.marching_cubes([[0.0]], 0.0)


# ---- 4. PLY writer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('coloured', [False, True])
def test_write_ply(tmp_path, coloured):
    from poseprobe_amd import mesh
    v = np.array([[0, 0, 0], [1, 0, 0.5], [0, 1, 0], [0.25, 0, 1]], np.float64)
    t = np.array([[0, 1, 2], [0, 3, 1]], np.int64)
    col = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]], np.uint8) if coloured else None
    path = tmp_path / 'm.ply'
    mesh.write_ply(str(path), torch.tensor(v), t, col)
    raw = path.read_bytes()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').splitlines()
    assert lines[:3] == ['ply', 'format binary_little_endian 1.0', 'element vertex 4']
    props = ['property float x', 'property float y', 'property float z']
    props += ['property uchar red', 'property uchar green', 'property uchar blue'] if coloured else []
    assert lines[3:] == props + ['element face 2', 'property list uchar int vertex_indices']
    vfmt = '<fffBBB' if coloured else '<fff'
    vsize = struct.calcsize(vfmt)
    assert len(body) == 4 * vsize + 2 * 13
    for i in range(4):
        rec = struct.unpack_from(vfmt, body, i * vsize)
        assert rec[:3] == tuple(np.float32(v[i])) and (not coloured or rec[3:] == tuple(col[i]))
    for i in range(2):
        assert struct.unpack_from('<Biii', body, 4 * vsize + 13 * i) == (3, *t[i])


# ---- 5. legacy names keep refusing ---------------------------------------------------------------------------------------------
def test_legacy_names_still_refuse_and_point_to_the_mesh_module():
    from poseprobe_amd import dvgo_ori, voxurf_coarse
    calls = [lambda: dvgo_ori.extract_geometry(torch.zeros(3), torch.ones(3), 5, 0.0, lambda p: p.sum(-1)),
             lambda: dvgo_ori.DirectVoxGO.extract_geometry(None, None, None),
             lambda: voxurf_coarse.Voxurf.extract_geometry(None, None, None),
             lambda: voxurf_coarse.Voxurf.extract_deform_geometry(None, None, None)]
    for f in calls:
        with pytest.raises(NotImplementedError, match='poseprobe_amd.mesh'):
            f()


def test_committed_table_header_is_what_the_generator_writes():
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('gen_mc_table', os.path.join(root, 'tools', 'gen_mc_table.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    table = gen.generate()
    assert open(gen.OUT).read() == gen.render(table)
    assert [[tuple(t) for t in row] for row in table] == rows()          # and the library was built from it
