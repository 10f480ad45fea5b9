"""DTU mesh evaluation, the part that needs no GPU: the numpy restatement of its semantics (tests/dtu_eval_reference.py - the
reference the GPU tests compare with) against a recorded run of the reference's own lib/dtu_eval.py::eval
(tests/golden/dtu_eval_synth.npz, written by tools/make_dtu_eval_golden.py) and, where sklearn exists, against the reference's own
neighbour calls; the round-based thinning against the sequential loop; the PLY reader; and the argument validation of the pp_dtu_*
entry points (every refusal comes before a launch)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import dtu_eval_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dtu_eval_synth.npz')
# Relative tolerance of the three means against the reference's float64 run: ten times the largest relative difference observed
# when the fixture was made (6.557e-08: float32 points and distances against float64), with a floor of 1e-6.
MEAN_RTOL = 1e-6
MODES = [('std', False), ('rt', True)]


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def restated(tag):
    g = golden()
    return R.chamfer(g['vertices'], g['triangles'], g['stl'], g['obs_mask'], g['bb'], g['res'], g['plane'],
                     runtime=dict(MODES)[tag], perm=g[f'perm_{tag}'])


def test_fixture_samples_triangle_interiors_in_both_modes():
    g = golden()
    referenced = len(np.unique(g['triangles']))
    for tag, _ in MODES:
        assert g[f'counts_{tag}'][0] > referenced + len(g['triangles'])


@pytest.mark.parametrize('tag', ['std', 'rt'])
def test_restatement_keeps_the_references_points_and_means(tag):
    g, r = golden(), restated(tag)
    assert [r['n_sampled'], r['n_down'], r['n_in_obs'], r['n_stl_above']] == g[f'counts_{tag}'].tolist()
    assert np.array_equal(r['down'], g[f'down_{tag}'])
    for name, want in zip(('mean_d2s', 'mean_s2d', 'over_all'), g[f'means_{tag}']):
        rel = abs(r[name] - want) / abs(want)
        print(f'{tag} {name}: {r[name]!r} against {want!r}, relative difference {rel:.3e}')
        assert rel <= MEAN_RTOL


@pytest.mark.parametrize('n,radius,seed', [(1, 0.5, 0), (300, 0.12, 1), (800, 0.09, 2)])
def test_restated_thinning_against_sklearn_radius_neighbors(n, radius, seed):
    skln = pytest.importorskip('sklearn.neighbors')
    p = np.random.RandomState(seed).rand(n, 3).astype(np.float32)
    d = np.sqrt(((p[:, None].astype(np.float64) - p[None].astype(np.float64)) ** 2).sum(-1))
    assert np.abs(d - radius)[d > 0].min() > 1e-6 if n > 1 else True, 'a pair sits on the radius: pick another seed'
    nn = skln.NearestNeighbors(n_neighbors=1, radius=radius, algorithm='kd_tree')
    nn.fit(p)
    mask = np.ones(n, bool)
    for curr, idxs in enumerate(nn.radius_neighbors(p, radius=radius, return_distance=False)):
        if mask[curr]:
            mask[idxs] = 0
            mask[curr] = 1
    assert np.array_equal(R.thin_points(p, radius), mask)
    assert 0 < mask.sum() < n or n == 1


def test_restated_nearest_against_sklearn_kneighbors():
    skln = pytest.importorskip('sklearn.neighbors')
    rs = np.random.RandomState(3)
    p, q = rs.rand(700, 3).astype(np.float32), (rs.rand(500, 3) * 1.4 - 0.2).astype(np.float32)
    nn = skln.NearestNeighbors(n_neighbors=1, algorithm='kd_tree')
    nn.fit(p)
    dist, _ = nn.kneighbors(q, n_neighbors=1, return_distance=True)
    d2, idx = R.nearest(q, p, 0.25)
    hit = dist[:, 0] < 0.25
    assert np.abs(dist[:, 0] - 0.25).min() > 1e-6 and hit.any() and not hit.all()
    assert np.array_equal(idx >= 0, hit) and np.isinf(d2[~hit]).all()
    assert np.allclose(np.sqrt(d2[hit].astype(np.float64)), dist[hit, 0], rtol=1e-6, atol=0)        # (by distance: ties may differ)


@pytest.mark.parametrize('n,radius,seed', [(1, 0.3, 0), (64, 0.5, 1), (700, 0.1, 2), (1500, 0.08, 3)])
def test_round_based_thinning_equals_the_sequential_loop(n, radius, seed):
    p = np.random.RandomState(seed).rand(n, 3).astype(np.float32)
    if n == 64:                                  # a chain in index order: every point waits for its predecessor
        p = np.zeros((n, 3), np.float32)
        p[:, 0] = np.arange(n) * np.float32(0.9 * radius)
    mask, rounds = R.thin_points_rounds(p, radius)
    assert np.array_equal(mask, R.thin_points(p, radius))
    if n == 64:
        assert rounds == 64 and np.array_equal(mask, np.arange(n) % 2 == 0)
    print(f'n={n}: kept {mask.sum()} in {rounds} rounds')


def test_thinning_radius_is_inclusive():
    r = np.float32(0.25)
    p = np.array([[0, 0, 0], [r, 0, 0], [0, 5, 0], [np.nextafter(r, np.float32(1)), 5, 0]], np.float32)
    assert R.thin_points(p, r).tolist() == [True, False, True, True]


@pytest.mark.parametrize('with_faces', [True, False])
def test_read_ply_reads_what_write_ply_writes_and_its_ascii_twin(tmp_path, with_faces):
    from poseprobe_amd import mesh
    v, t = R.icosphere(1)
    v = (v * 3.7 - 1.2).astype(np.float32)
    t = t if with_faces else np.empty((0, 3), np.int32)
    colors = (np.arange(3 * len(v)) % 251).astype(np.uint8).reshape(-1, 3)
    mesh.write_ply(tmp_path / 'b.ply', v, t, vertex_colors=colors)
    header = ['ply', 'format ascii 1.0', 'comment made by a test', f'element vertex {len(v)}', 'property double x',
              'property double y', 'property double z', 'property uchar red', f'element face {len(t)}',
              'property list uchar int vertex_indices', 'end_header']
    rows = [f'{float(a)!r} {float(b)!r} {float(c)!r} {k % 200}' for k, (a, b, c) in enumerate(v)] + [f'3 {a} {b} {c}' for a, b, c in t]
    (tmp_path / 'a.ply').write_text('\n'.join(header + rows) + '\n')
    for name, dtype in (('b.ply', np.float32), ('a.ply', np.float64)):
        v2, t2 = mesh.read_ply(tmp_path / name)
        assert v2.dtype == dtype and t2.dtype == np.int32 and t2.shape == (len(t), 3)
        assert np.array_equal(v2, v.astype(dtype)) and np.array_equal(t2, t)
    (tmp_path / 'c.ply').write_bytes(b'ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nend_header\n')
    with pytest.raises(ValueError, match='binary_big_endian'):
        mesh.read_ply(tmp_path / 'c.ply')
    with pytest.raises(ValueError, match='not a PLY'):
        mesh.read_ply(GOLDEN)


# ---- argument validation (before any GPU call) --------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)         # never dereferenced: every call below is refused first
GRID = (0.0, 0.0, 0.0, 0.5, 8, 8, 8)
BAD_GRIDS = [(float('nan'), 0.0, 0.0, 0.5, 8, 8, 8), (0.0, float('inf'), 0.0, 0.5, 8, 8, 8), (0.0, 0.0, 0.0, 0.0, 8, 8, 8),
             (0.0, 0.0, 0.0, -1.0, 8, 8, 8), (0.0, 0.0, 0.0, float('nan'), 8, 8, 8), (0.0, 0.0, 0.0, 0.5, 0, 8, 8),
             (0.0, 0.0, 0.0, 0.5, 8, -1, 8), (0.0, 0.0, 0.0, 0.5, 8, 8, 0)]


def _refused(rc, name, code=-1):
    from poseprobe_amd import _lib
    assert rc == code, (name, rc)
    assert name.encode() in _lib.lib().pp_last_error()


def _each_null(call, names, name, optional=()):
    from poseprobe_amd import _lib
    for n in names:
        if n not in optional:
            _refused(call(**{n: None}), name)
            assert b'null' in _lib.lib().pp_last_error()


@pytest.mark.parametrize('entry', ['pp_dtu_sample_count', 'pp_dtu_sample_emit'])
def test_sampling_entry_points_validate_before_any_gpu_call(entry):
    from poseprobe_amd import _lib
    L = _lib.lib()
    names = ('vertices', 'triangles', 'counts') if entry.endswith('count') else ('vertices', 'triangles', 'offsets', 'points')

    def call(V=8, T=4, thresh=0.2, n_points=16, **ptr):
        a = {n: FAKE for n in names}
        a.update(ptr)
        if entry.endswith('count'):
            return L.pp_dtu_sample_count(a['vertices'], V, a['triangles'], T, thresh, a['counts'], None)
        return L.pp_dtu_sample_emit(a['vertices'], V, a['triangles'], T, thresh, a['offsets'], a['points'], n_points, None)

    _each_null(call, names, entry)
    for kw in (dict(V=0), dict(V=-3), dict(T=0), dict(T=-1), dict(thresh=0.0), dict(thresh=-0.2), dict(thresh=float('nan')),
               dict(thresh=float('inf'))):
        _refused(call(**kw), entry)
    if entry.endswith('emit'):
        _refused(call(n_points=-1), entry)
        _refused(call(n_points=2 ** 31), entry, -3)
        assert call(n_points=0, points=None) == 0                     # nothing to write: no launch


def test_cell_keys_validates_before_any_gpu_call():
    from poseprobe_amd import _lib
    L = _lib.lib()

    def call(N=16, grid=GRID, **ptr):
        a = dict(points=FAKE, keys=FAKE)
        a.update(ptr)
        return L.pp_dtu_cell_keys(a['points'], N, *grid, a['keys'], None)

    _each_null(call, ('points', 'keys'), 'pp_dtu_cell_keys')
    for N in (0, -1):
        _refused(call(N=N), 'pp_dtu_cell_keys')
    for g in BAD_GRIDS:
        _refused(call(grid=g), 'pp_dtu_cell_keys')
    _refused(call(grid=(0.0, 0.0, 0.0, 0.5, 8, 2 ** 20 + 1, 8)), 'pp_dtu_cell_keys', -3)


def test_thin_workspace_values_and_refusals():
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    b = ctypes.c_int64(-1)
    _refused(L.pp_dtu_thin_workspace(16, None), 'pp_dtu_thin_workspace')
    for N in (0, -1):
        _refused(L.pp_dtu_thin_workspace(N, ctypes.byref(b)), 'pp_dtu_thin_workspace')
    assert b.value == -1
    assert [ops.dtu_thin_workspace(N) for N in (1, 256, 257, 5000)] == [512, 512, 1024, 2 * 5120]


def test_thin_rounds_validates_before_any_gpu_call():
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    N = 300
    need = ops.dtu_thin_workspace(N)
    names = ('points', 'keys', 'order', 'work', 'undecided')

    def call(N=N, grid=GRID, radius=0.4, first=0, n_rounds=4, work_bytes=need, **ptr):
        a = {n: FAKE for n in names}
        a.update(ptr)
        return L.pp_dtu_thin_rounds(a['points'], a['keys'], a['order'], N, *grid, radius, first, n_rounds, a['work'], work_bytes,
                                    a['undecided'], None)

    _each_null(call, names, 'pp_dtu_thin_rounds')
    for kw in (dict(N=0), dict(N=-2), dict(radius=-0.1), dict(radius=float('nan')), dict(radius=0.6), dict(first=-1),
               dict(n_rounds=0), dict(n_rounds=1025)):
        _refused(call(**kw), 'pp_dtu_thin_rounds')
    for g in BAD_GRIDS:
        _refused(call(grid=g), 'pp_dtu_thin_rounds')
    _refused(call(work_bytes=need - 1), 'pp_dtu_thin_rounds')
    assert b'workspace' in L.pp_last_error()


def test_nearest_validates_before_any_gpu_call():
    from poseprobe_amd import _lib
    L = _lib.lib()
    names = ('queries', 'points', 'keys', 'order', 'd2', 'idx')

    def call(Q=10, P=20, grid=GRID, max_dist=2.0, **ptr):
        a = {n: FAKE for n in names}
        a.update(ptr)
        return L.pp_dtu_nearest(a['queries'], Q, a['points'], a['keys'], a['order'], P, *grid, max_dist, a['d2'], a['idx'], None)

    _each_null(call, names, 'pp_dtu_nearest')
    for kw in (dict(Q=0), dict(Q=-1), dict(P=0), dict(P=-5), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float('nan')),
               dict(max_dist=float('inf'))):
        _refused(call(**kw), 'pp_dtu_nearest')
    for g in BAD_GRIDS:
        _refused(call(grid=g), 'pp_dtu_nearest')


def test_wrappers_refuse_cpu_tensors_and_wrong_shapes():
    import torch
    from poseprobe_amd import dtu_eval
    p = torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match='CUDA'):
        dtu_eval.thin_points(p, 0.2)
    with pytest.raises(RuntimeError, match='CUDA'):
        dtu_eval.nearest(p, p, 1.0)
    with pytest.raises(RuntimeError, match='CUDA'):
        dtu_eval.sample_mesh_points(p.double(), torch.zeros(1, 3, dtype=torch.int32), 0.2)
    with pytest.raises(TypeError):
        dtu_eval.thin_points(np.zeros((4, 3), np.float32), 0.2)


def test_validate_mesh_refuses_vertex_colours():
    from poseprobe_amd import dtu_eval
    with pytest.raises(NotImplementedError, match='extract_color'):
        dtu_eval.validate_mesh(None, None, extract_color=True)
