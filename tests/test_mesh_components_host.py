"""Host-side checks of the mesh-cleaning feature (poseprobe_amd.mesh.connected_components / keep_components,
csrc/pp_mesh_components.hip): the numpy restatement the GPU tests compare against (tests/mesh_components_reference.py) is checked
against scipy and against mathematics, the refusals that need no GPU, the header and the ABI.  No test here needs a GPU."""
import numpy as np
import pytest
import torch

from poseprobe_amd import mesh, ops
from tests import mesh_components_reference as R
from tests import mesh_reference as M

# The restatement is the yardstick of the feature and has no other use: this module needs the feature's public names, and
# without them none of its tests runs - the checks of the restatement included.
FEATURE = (mesh.connected_components, mesh.keep_components, mesh.CC_BATCH, mesh.CC_MAX_BATCHES, ops.cc_workspace, ops.cc_rounds,
           ops.cc_count, ops.cc_keep_masks, ops.cc_compact)

MESHES = ('three_body', 'noise', 'big_and_small')
STRIPS = ('ascending', 'descending', 'random')


def _all_cases():
    cases = dict(R.small_cases())
    for name in MESHES:
        v, t = R.mc_mesh(name)
        cases[name] = (t, len(v))
    for numbering in STRIPS:
        cases['strip_' + numbering] = R.strip(R.STRIP_TRIANGLES, numbering)
    return cases


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(_all_cases()))
def test_restatement_agrees_with_scipy(name):
    csgraph = pytest.importorskip('scipy.sparse.csgraph')
    sparse = pytest.importorskip('scipy.sparse')
    t, nv = _all_cases()[name]
    cc = R.connected_components(t, nv)
    t64 = np.asarray(t, dtype=np.int64).reshape(-1, 3)
    rows, cols = np.concatenate([t64[:, 0], t64[:, 0]]), np.concatenate([t64[:, 1], t64[:, 2]])
    graph = sparse.coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(nv, nv))
    n, comp = csgraph.connected_components(graph, directed=False) if nv else (0, np.empty(0, np.int64))
    referenced = np.zeros(nv, dtype=bool)
    referenced[t64.reshape(-1)] = True
    assert n - int((~referenced).sum()) == cc['n_components']           # scipy counts every unreferenced vertex as a component
    lab = cc['labels']
    assert ((lab == -1) == ~referenced).all()
    # the same partition, and the label is the smallest index of the part
    smallest = np.full(max(n, 1), nv, dtype=np.int64)
    np.minimum.at(smallest, comp[referenced], np.flatnonzero(referenced))
    assert np.array_equal(lab[referenced], smallest[comp[referenced]])
    assert np.array_equal(cc['roots'], np.unique(lab[referenced]))
    assert cc['vertex_counts'].sum() == referenced.sum() and cc['triangle_counts'].sum() == len(t64)
    assert cc['labels'].dtype == cc['roots'].dtype == np.int32


def test_restatement_on_the_small_cases_by_hand():
    c = R.small_cases()
    cc = R.connected_components(*c['no_triangle'])
    assert cc['n_components'] == 0 and (cc['labels'] == -1).all() and len(cc['roots']) == 0
    assert R.connected_components(*c['one_triangle'])['labels'].tolist() == [0, 0, 0]
    assert R.connected_components(*c['two_disjoint'])['labels'].tolist() == [0, 0, 0, 3, 3, 3]
    cc = R.connected_components(*c['shared_vertex'])
    assert cc['labels'].tolist() == [0] * 5 and cc['triangle_counts'].tolist() == [2] and cc['vertex_counts'].tolist() == [5]
    cc = R.connected_components(*c['unreferenced'])
    assert cc['labels'].tolist() == [-1, -1, 2, 2, -1, 2, 6, -1, 2, 2, -1, 6, 6, 6, -1, -1]
    assert cc['roots'].tolist() == [2, 6] and cc['vertex_counts'].tolist() == [5, 4] and cc['triangle_counts'].tolist() == [2, 2]


@pytest.mark.parametrize('name', sorted(_all_cases()))
def test_round_schedule_reaches_the_same_labels(name):
    """The restated schedule of the kernels (hook on a snapshot, a bounded jump) ends in the union-find's labels; the strips need
    more rounds than one batch of the host loop, which is what makes them exercise that loop on the GPU."""
    t, nv = _all_cases()[name]
    lab, rounds = R.rounds(t, nv)
    assert np.array_equal(lab, R.labels(t, nv))
    assert rounds <= mesh.CC_BATCH * mesh.CC_MAX_BATCHES // 8
    if name.startswith('strip_'):
        assert rounds > mesh.CC_BATCH, (name, rounds)
        assert R.rounds(t, nv, hops=1)[1] > rounds                      # fewer hops, more rounds: the count really is the schedule's


def test_three_bodies_have_the_euler_characteristics_of_two_spheres_and_a_torus():
    v, t = R.mc_mesh('three_body')
    cc = R.connected_components(t, len(v))
    assert cc['n_components'] == 3
    for root in cc['roots']:
        sub, n = R.component_mesh(cc, t, root)
        assert M.is_closed_manifold(sub, n)
        is_torus = v[cc['labels'] == root][:, 2].mean() < 9               # the torus lies in the low z layers
        assert M.euler_characteristic(sub, n) == (0 if is_torus else 2)
    assert R.connected_components(R.mc_mesh('noise')[1], len(R.mc_mesh('noise')[0]))['n_components'] > 100


def test_restated_filter_keeps_exactly_the_big_sphere():
    """keep='largest' on the mesh of max(u_big, u_small) is, bit for bit, the mesh of u_big alone: the spheres are 6.6 cells apart,
    so every cell the big sphere's surface crosses sees u_big only, and dropping the small sphere's vertices leaves the canonical
    order of the others."""
    gap = np.linalg.norm(R.BIG['c'] - R.SMALL['c']) - R.BIG['r'] - R.SMALL['r']
    assert gap > 2
    vb, tb = R.mc_mesh('big')
    M.sphere_checks(vb, tb, R.BIG['c'], R.BIG['r'])
    v, t = R.mc_mesh('big_and_small')
    assert len(v) > len(vb)
    k = R.keep_components(v, t, 'largest')
    assert np.array_equal(k['vertices'], vb) and np.array_equal(k['triangles'], tb)
    assert k['n_components'] == 2 and k['n_kept'] == 1 and np.array_equal(v[k['vertex_index']], vb)


def test_restated_keep_rules():
    v, t = R.mc_mesh('noise')
    cc = R.connected_components(t, len(v))
    tc = cc['triangle_counts']
    assert R.kept_roots(cc, 'largest').tolist() == [int(cc['roots'][np.argmax(tc)])]
    assert set(R.kept_roots(cc, 8)) == set(cc['roots'][tc >= 8]) and 1 < len(R.kept_roots(cc, 8)) < cc['n_components']
    assert len(R.kept_roots(cc, 0)) == cc['n_components'] and len(R.kept_roots(cc, 10 ** 9)) == 0
    assert R.kept_roots(cc, 0.5).tolist() == R.kept_roots(cc, 'largest').tolist()
    tie = R.connected_components(*R.small_cases()['two_disjoint'])
    assert R.kept_roots(tie, 'largest').tolist() == [0]                    # ties go to the lowest root
    k = R.keep_components(np.arange(18, dtype=np.float32).reshape(6, 3), R.small_cases()['two_disjoint'][0], 1,
                          attributes=dict(a=np.arange(6)))
    assert k['triangles'].tolist() == [[0, 1, 2], [3, 4, 5]] and k['a'].tolist() == list(range(6))


# ---- refusals that need no GPU ------------------------------------------------------------------------------------------------------
def test_triangle_indices_out_of_range_are_refused():
    for bad in ([[0, 1, 3]], [[0, -1, 2]], [[0, 1, 2], [2, 1, 7]]):
        with pytest.raises(ValueError, match='index vertices'):
            mesh.connected_components(np.array(bad, dtype=np.int32), 3)
        with pytest.raises(ValueError, match='index vertices'):
            mesh.keep_components(np.zeros((3, 3), np.float32), np.array(bad, dtype=np.int64))
    with pytest.raises(ValueError, match='negative'):
        mesh.connected_components(np.zeros((0, 3), np.int32), -1)


def test_wrong_types_and_shapes_are_refused():
    with pytest.raises(TypeError, match='triangles'):
        mesh.connected_components([[0, 1, 2]], 3)
    with pytest.raises(TypeError, match='integers'):
        mesh.connected_components(np.zeros((1, 3), np.float32), 3)
    with pytest.raises(TypeError, match='int32'):
        mesh.connected_components(torch.zeros(1, 3, dtype=torch.int64), 3)
    with pytest.raises(TypeError, match='int32'):
        mesh.connected_components(torch.zeros(1, 3, dtype=torch.float32), 3)
    for shape in ((3,), (1, 4), (1, 3, 1)):
        with pytest.raises(ValueError, match=r'\[Nt, 3\]'):
            mesh.connected_components(np.zeros(shape, np.int32), 3)
        with pytest.raises(ValueError, match=r'\[Nt, 3\]'):
            mesh.connected_components(torch.zeros(shape, dtype=torch.int32), 3)
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        mesh.connected_components(torch.zeros(1, 3, dtype=torch.int32), 3)
    tri = np.array([[0, 1, 2]], dtype=np.int32)
    with pytest.raises(TypeError, match='vertices'):
        mesh.keep_components([[0., 0., 0.]] * 3, tri)
    with pytest.raises(TypeError, match='floats'):
        mesh.keep_components(np.zeros((3, 3), np.int32), tri)
    with pytest.raises(ValueError, match=r'\[Nv, 3\]'):
        mesh.keep_components(np.zeros((3, 2), np.float32), tri)
    with pytest.raises(ValueError, match='one row per vertex'):
        mesh.keep_components(np.zeros((3, 3), np.float32), tri, attributes=dict(colors=np.zeros((2, 3))))
    with pytest.raises(ValueError, match="result's own"):
        mesh.keep_components(np.zeros((3, 3), np.float32), tri, attributes=dict(vertices=np.zeros((3, 3))))


@pytest.mark.parametrize('keep,error', [('biggest', ValueError), ('', ValueError), (None, TypeError), (True, TypeError), ([1], TypeError),
                                        (-1, ValueError), (0.0, ValueError), (1.0, ValueError), (1.5, ValueError), (-0.25, ValueError),
                                        (float('nan'), ValueError)])
def test_unknown_keep_rules_are_refused(keep, error):
    with pytest.raises(error, match='keep'):
        mesh.keep_components(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], dtype=np.int32), keep=keep)


# ---- header and ABI ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_and_the_abi_stays():
    from poseprobe_amd import _lib
    protos = _lib.parse_header()
    names = lambda f: [n for _, n in protos[f]]
    assert names('pp_cc_workspace') == ['n_vertices', 'bytes']
    assert names('pp_cc_rounds') == ['triangles', 'n_triangles', 'n_vertices', 'first_round', 'n_rounds', 'labels', 'work', 'work_bytes',
                                     'changed', 'stream']
    assert names('pp_cc_count') == ['labels', 'n_vertices', 'triangles', 'n_triangles', 'vertex_counts', 'triangle_counts', 'stream']
    assert names('pp_cc_keep_masks') == ['labels', 'n_vertices', 'triangles', 'n_triangles', 'root_keep', 'vertex_keep', 'triangle_keep',
                                         'stream']
    assert names('pp_cc_compact') == ['vertices', 'triangles', 'vertex_scan', 'triangle_scan', 'n_vertices', 'n_triangles', 'out_vertices',
                                      'out_index', 'out_triangles', 'n_out_vertices', 'n_out_triangles', 'stream']
    assert _lib.header_abi_version() == 4
    assert _lib.OPTION_NAMES == ('mlp_fused', 'grid_chunks', 'nerf_split', 'mlp_split', 'mlp_wgs', 'nerf_chain', 'mlp_pack', 'warp_lean')


def test_library_refuses_bad_arguments_before_any_gpu_call():
    """The entry points check their arguments on the host (PP_REQUIRE): these calls fail without a GPU in the machine."""
    import ctypes
    from poseprobe_amd import _lib
    L = _lib.lib()
    assert L.pp_abi_version() == 4
    b = ctypes.c_int64(-1)
    assert L.pp_cc_workspace(1000, ctypes.byref(b)) == 0 and b.value == 2 * 4096
    assert L.pp_cc_workspace(0, ctypes.byref(b)) == 0 and b.value == 0
    assert L.pp_cc_workspace(-1, ctypes.byref(b)) == -1 and b'negative' in L.pp_last_error()
    assert L.pp_cc_workspace((1 << 30) + 1, ctypes.byref(b)) == -3
    assert L.pp_cc_workspace(5, None) == -1
    one = ctypes.c_void_p(256)                         # never dereferenced: every call below is refused first
    assert L.pp_cc_rounds(one, 1, 3, 0, 0, one, one, 1 << 20, one, None) == -1 and b'n_rounds' in L.pp_last_error()
    assert L.pp_cc_rounds(one, 1, 3, 0, 1025, one, one, 1 << 20, one, None) == -1
    assert L.pp_cc_rounds(one, 1, 3, -1, 4, one, one, 1 << 20, one, None) == -1
    assert L.pp_cc_rounds(one, 1, 3, 0, 4, one, one, 1 << 20, None, None) == -1 and b'null' in L.pp_last_error()
    assert L.pp_cc_rounds(None, 1, 3, 0, 4, one, one, 1 << 20, one, None) == -1
    assert L.pp_cc_rounds(one, 1, 3, 0, 4, None, one, 1 << 20, one, None) == -1
    assert L.pp_cc_rounds(one, 1, 3, 0, 4, one, one, 511, one, None) == -1 and b'workspace' in L.pp_last_error()
    assert L.pp_cc_rounds(one, -1, 3, 0, 4, one, one, 1 << 20, one, None) == -1
    assert L.pp_cc_count(None, 3, one, 1, one, one, None) == -1
    assert L.pp_cc_count(one, 3, None, 1, one, one, None) == -1
    assert L.pp_cc_keep_masks(one, 3, one, 1, None, one, one, None) == -1
    assert L.pp_cc_keep_masks(one, 3, one, 1, one, one, None, None) == -1
    assert L.pp_cc_compact(one, one, one, one, 3, 1, one, one, one, 4, 1, None) == -1 and b'kept row counts' in L.pp_last_error()
    assert L.pp_cc_compact(one, one, one, one, 3, 1, one, one, one, 0, 1, None) == -1
    assert L.pp_cc_compact(one, one, one, one, 3, 1, None, one, one, 3, 1, None) == -1
    assert L.pp_cc_compact(None, one, one, one, 3, 1, one, one, one, 3, 1, None) == -1
