"""DTU mesh evaluation on the GPU (poseprobe_amd.dtu_eval, csrc/pp_dtu_eval.hip) against the numpy restatement of its semantics
(tests/dtu_eval_reference.py, itself checked against a recorded run of the reference in tests/test_dtu_eval_host.py): the three
stages one at a time on their edge cases, then the metric end to end on the recorded scene.

Near-ties in the sampling.  The single triangles are chosen so that no l / thr lies within 1e-6 of an integer and no barycentric
sum a + b within 1e-9 of 1, and the test asserts it, so that a near-tie cannot hide a wrong decision.  Two inputs cannot meet
that and are kept WITHOUT the assertion on the sums, because they decide a tie only if the device arithmetic is bit-equal to
numpy's, which is the stronger check: the icospheres (a nearly equilateral triangle has n1 == n2 = n, and then a + b is 1 up to
rounding for every i + j = n - 1; their l / thr still keep the 1e-6), and the right triangle with exactly unit legs at thresh 0.2
(l / thr is 5 up to rounding)."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dtu_eval_reference as R
from tests.test_dtu_eval_host import GOLDEN, MEAN_RTOL, MODES

pytestmark = pytest.mark.gpu

DEV = 'cuda'
T0 = [[0, 1, 2]]
# name: (vertices, triangles, thresh)
SINGLE = {
    'n1 = n2 = 0': ([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], T0, 0.2),
    'n1 = 1': ([[1, 2, 3], [1.3, 2, 3], [1, 2.5, 3]], T0, 0.2),
    'right, legs near 1': ([[0, 0, 0], [1.03, 0, 0], [0, 0.97, 0]], T0, 0.2),
    'sliver': ([[-1, 0, 2], [2.1, 0, 2], [0.7, 0.31, 2]], T0, 0.2),
    'zero area': ([[0, 0, 0], [1, 1, 1], [2, 2, 2]], T0, 0.2),
    'n about 40': ([[0.5, -3, 1], [8.6, -3, 1.2], [0.3, 4.9, 0.8]], T0, 0.2),
    'n about 40, thresh 0.5': ([[0.5, -3, 1], [20.7, -3, 1.2], [0.3, 16.9, 0.8]], T0, 0.5),
    'unreferenced vertex': ([[9, 9, 9], [0, 0, 0], [1.03, 0, 0], [7, 7, 7], [0, 0.97, 0]], [[1, 2, 4], [4, 2, 1]], 0.2),
    'two triangles and a zero-area one between': ([[0, 0, 0], [1.03, 0, 0], [0, 0.97, 0], [2.06, 0, 0], [1.1, 1.3, 0.2]],
                                                  [[0, 1, 2], [0, 1, 3], [1, 3, 4]], 0.2),
}
TIED = {
    'right, unit legs': ([[0, 0, 0], [1, 0, 0], [0, 1, 0]], T0, 0.2),
    'icosphere 320': (None, 2, 0.2),
    'icosphere 1280': (None, 3, 0.2),
}


def dev(a, dtype):
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


@functools.lru_cache(maxsize=None)
def sampling_case(name):
    v, t, thresh = {**SINGLE, **TIED}[name]
    if v is None:
        v, t = R.icosphere(t)
        v = (v * np.array([5.9, 6.3, 6.1]) + 10.0).astype(np.float32)
    v, t = np.asarray(v, np.float64), np.asarray(t, np.int32)
    info = {}
    want = R.sample_mesh_points(v, t, thresh, info)
    want.setflags(write=False)
    return v, t, thresh, want, info


@pytest.mark.parametrize('name', list(SINGLE) + list(TIED))
def test_sampling_count_order_and_coordinates(name):
    from poseprobe_amd import dtu_eval
    v, t, thresh, want, info = sampling_case(name)
    print(f'{name}: {len(want)} points, n = {info["n"][:3]}, l / thr at least {info["count_margin"]:.2e} from an integer, '
          f'a + b at least {info["sum_margin"]:.2e} from 1')
    if name != 'right, unit legs':
        assert info['count_margin'] > 1e-6
    if name in SINGLE:
        assert info['sum_margin'] > 1e-9
    got = dtu_eval.sample_mesh_points(dev(v, torch.float64), dev(t, torch.int32), thresh)
    assert got.dtype == torch.float32 and got.is_cuda
    got = got.cpu().numpy()
    assert got.shape == want.shape                                         # the count
    ulp = np.spacing(np.abs(want))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f'{name}: bit-equal to the restatement: {np.array_equal(got, want)}; largest error {float((err / ulp).max()) if len(want) else 0.0} ulp')
    assert (err <= ulp).all()                                              # the order, and every coordinate within one float32 ulp


def test_sampling_cases_cover_what_they_name():
    n = lambda name: sampling_case(name)[4]['n']
    assert n('n1 = n2 = 0') == [(0, 0)] and n('n1 = 1') == [(1, 2)] and n('zero area') == []
    assert n('right, unit legs') == [(5, 5)] and n('right, legs near 1') == [(5, 4)]
    assert min(n('n about 40')[0]) >= 39 and len(sampling_case('n about 40')[3]) > 750
    assert len(sampling_case('n1 = n2 = 0')[3]) == 3 and len(sampling_case('zero area')[3]) == 3
    v, _, _, want, _ = sampling_case('unreferenced vertex')
    assert np.array_equal(want[:3], v[[1, 2, 4]].astype(np.float32)) and not (want == 9).all(1).any() and not (want == 7).all(1).any()


def test_sampling_refuses_bad_indices_and_accepts_an_empty_mesh():
    from poseprobe_amd import dtu_eval
    v = dev(SINGLE['sliver'][0], torch.float64)
    with pytest.raises(ValueError, match='index'):
        dtu_eval.sample_mesh_points(v, dev([[0, 1, 3]], torch.int32), 0.2)
    assert dtu_eval.sample_mesh_points(v, torch.empty(0, 3, dtype=torch.int32, device=DEV), 0.2).shape == (0, 3)


def test_sampling_emit_writes_the_rows_it_is_given_and_nothing_past_them():
    """pp_dtu_sample_emit with fewer rows than were counted: the first rows of the full result inside 64 KB of sentinel bytes."""
    from poseprobe_amd import ops
    v, t, thresh, want, _ = sampling_case('icosphere 320')
    want = want[len(np.unique(t)):]                                        # (the sampled points; the vertices are the host's)
    vd, td = dev(v, torch.float64), dev(t, torch.int32)
    counts = torch.empty(len(t), dtype=torch.int64, device=DEV)
    ops.dtu_sample_count(vd, td, thresh, counts)
    assert int(counts.sum()) == len(want)
    offsets = (torch.cumsum(counts, 0) - counts).contiguous()
    guard = 65536
    for n in (len(want), len(want) - 1, 1000, 1):
        buf = torch.full((2 * guard + 12 * n,), 0xA5, dtype=torch.uint8, device=DEV)
        ops.dtu_sample_emit(vd, td, thresh, offsets, buf[guard:guard + 12 * n].view(torch.float32).view(n, 3), n)
        got = buf.cpu().numpy()
        assert (got[:guard] == 0xA5).all() and (got[guard + 12 * n:] == 0xA5).all()
        assert np.array_equal(got[guard:guard + 12 * n].view(np.float32).reshape(n, 3), want[:n])


# ---- thinning -------------------------------------------------------------------------------------------------------------------------
RADIUS = np.float32(0.25)


def thinning_cases():
    rs = np.random.RandomState(5)
    r = RADIUS
    beyond = np.nextafter(r, np.float32(1))
    edge = np.float32(r) * np.float32(1.01)
    k = rs.randint(-12, 0, size=(400, 3))
    borders = (k * edge + rs.choice([-1e-3, 1e-3, 0.0], size=(400, 3)) * edge + rs.rand(400, 1) * 0.05).astype(np.float32) - np.float32(0.7)
    cloud = rs.rand(5000, 3).astype(np.float32)
    chain = np.zeros((64, 3), np.float32)
    chain[:, 0] = np.arange(64) * np.float32(0.9 * r)
    return {
        'one point': (np.array([[1, 2, 3]], np.float32), r),
        'exactly at radius and just beyond': (np.array([[0, 0, 0], [r, 0, 0], [0, 5, 0], [beyond, 5, 0]], np.float32), r),
        'duplicates': (np.array([[1, 1, 1], [1, 1, 1], [4, 1, 1], [1, 1, 1], [4, 1, 1], [-3, 0, 2]], np.float32), r),
        'chain': (chain, r),
        'cell borders at negative coordinates': (borders, r),
        '5000 random, about three neighbours each': (cloud[rs.permutation(5000)], np.float32(0.0523)),
    }


@functools.lru_cache(maxsize=None)
def thinning_case(name):
    p, r = thinning_cases()[name]
    want = R.thin_points(p, r)
    want.setflags(write=False)
    return p, r, want


@pytest.mark.parametrize('name', list(thinning_cases()))
def test_thinning_mask_is_exactly_the_sequential_loops(name):
    from poseprobe_amd import dtu_eval
    p, r, want = thinning_case(name)
    info = {}
    got = dtu_eval.thin_points(dev(p, torch.float32), float(r), info)
    assert got.dtype == torch.bool and got.is_cuda
    print(f'{name}: {len(p)} points, {int(want.sum())} kept, {info["rounds"]} rounds')
    assert np.array_equal(got.cpu().numpy(), want)
    if name == 'exactly at radius and just beyond':
        assert want.tolist() == [True, False, True, True]
    if name == 'chain':
        assert info['rounds'] == 64 and np.array_equal(want, np.arange(64) % 2 == 0)
    if name.startswith('5000'):
        d = p[:, None, :] - p[None, :1000, :]
        assert 2.0 < ((d ** 2).sum(-1) <= r * r).sum() / 1000 - 1 < 4.5          # the mean number of neighbours
        assert info['rounds'] < 30
    if name == 'duplicates':
        assert want.tolist() == [True, False, True, False, False, True]
    assert dtu_eval.thin_points(torch.empty(0, 3, device=DEV), 0.2).shape == (0,)


# ---- nearest --------------------------------------------------------------------------------------------------------------------------
def nearest_cases():
    rs = np.random.RandomState(7)
    md = np.float32(2.0)
    inside = np.nextafter(md, np.float32(0))
    clusters = np.concatenate([rs.rand(50, 3) * 0.2, rs.rand(50, 3) * 0.2 + 10.0]).astype(np.float32)
    far_q = (np.array([[6, 10, 10], [5.5, 9, 11], [10, 10, 5.2], [4, 4, 4], [13, 13.5, 12]]) + rs.rand(5, 3) * 0.1).astype(np.float32)
    points = rs.rand(6000, 3).astype(np.float32)
    points[:2000] *= np.float32(0.3)                                              # uneven density
    queries = (rs.rand(4000, 3) * 1.6 - 0.3).astype(np.float32)
    queries[:20] = queries[:20] * 10 - 5                                           # a few far outside the cloud
    return {
        'P = Q = 1': (np.array([[0.5, 0.25, -1]], np.float32), np.array([[1, 2, 3]], np.float32), np.float32(20), None),
        'exact tie': (np.array([[0, 0, 0]], np.float32),
                      np.array([[3, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, -1], [-1, 0, 0], [0, 0, 2]], np.float32), md, None),
        'exactly at max_dist and just inside': (np.array([[0, 0, 0], [0, 7, 0]], np.float32),
                                                np.array([[md, 0, 0], [inside, 7, 0]], np.float32), md, None),
        'several rings to a distant cluster': (far_q, clusters, np.float32(20), 0.5),
        '4000 queries, 6000 points': (queries, points, np.float32(0.2), None),
    }


@functools.lru_cache(maxsize=None)
def nearest_case(name):
    q, p, md, edge = nearest_cases()[name]
    d2, idx = R.nearest(q, p, md)
    d2.setflags(write=False)
    idx.setflags(write=False)
    return q, p, md, edge, d2, idx


@pytest.mark.parametrize('name', list(nearest_cases()))
def test_nearest_index_and_distance_are_bit_equal(name):
    from poseprobe_amd import dtu_eval
    q, p, md, edge, d2, idx = nearest_case(name)
    got_d2, got_idx = dtu_eval.nearest(dev(q, torch.float32), dev(p, torch.float32), float(md), cell_edge=edge)
    assert got_d2.dtype == torch.float32 and got_idx.dtype == torch.int32
    print(f'{name}: {int((idx >= 0).sum())} of {len(q)} queries have a point within {md}')
    assert np.array_equal(got_idx.cpu().numpy(), idx)
    assert np.array_equal(got_d2.cpu().numpy().view(np.uint32), d2.view(np.uint32))
    if name == 'exact tie':
        assert idx.tolist() == [1]
    if name == 'exactly at max_dist and just inside':
        assert idx.tolist() == [-1, 1] and np.isinf(d2[0])
    if name == 'several rings to a distant cluster':
        assert (idx >= 50).sum() == 4 and idx[3] < 50 and (np.sqrt(d2) > 3).all()   # at least six rings of 0.5
    if name.startswith('4000'):
        assert 0 < (idx < 0).sum() < len(q) / 2


def test_nearest_does_not_depend_on_the_cell_edge():
    from poseprobe_amd import dtu_eval
    q, p, md, _, d2, idx = nearest_case('4000 queries, 6000 points')
    for edge in (0.037, 0.5):
        got_d2, got_idx = dtu_eval.nearest(dev(q, torch.float32), dev(p, torch.float32), float(md), cell_edge=edge)
        assert np.array_equal(got_idx.cpu().numpy(), idx) and np.array_equal(got_d2.cpu().numpy().view(np.uint32), d2.view(np.uint32))


def test_nearest_without_points_or_queries_launches_nothing():
    from poseprobe_amd import dtu_eval
    q = dev(np.zeros((5, 3)), torch.float32)
    d2, idx = dtu_eval.nearest(q, torch.empty(0, 3, device=DEV), 20.0)
    assert torch.isinf(d2).all() and (idx == -1).all() and d2.shape == idx.shape == (5,)
    d2, idx = dtu_eval.nearest(torch.empty(0, 3, device=DEV), q, 20.0)
    assert d2.shape == idx.shape == (0,)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def restated(tag):
    g = golden()
    return R.chamfer(g['vertices'], g['triangles'], g['stl'], g['obs_mask'], g['bb'], g['res'], g['plane'],
                     runtime=dict(MODES)[tag], perm=g[f'perm_{tag}'])


COUNTS = ('n_sampled', 'n_down', 'n_in_obs', 'n_stl_above')
MEANS = ('mean_d2s', 'mean_s2d', 'over_all')


@pytest.mark.parametrize('tag', ['std', 'rt'])
def test_chamfer_on_the_recorded_scene(tag):
    from poseprobe_amd import dtu_eval
    g, want = golden(), restated(tag)
    call = lambda: dtu_eval.chamfer(g['vertices'], g['triangles'], g['stl'], g['obs_mask'], g['bb'], g['res'], g['plane'],
                                    runtime=dict(MODES)[tag], perm=g[f'perm_{tag}'])
    got = call()
    assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS] == g[f'counts_{tag}'].tolist()
    for k, ref in zip(MEANS, g[f'means_{tag}']):
        print(f'{tag} {k}: {got[k]!r}, restatement {want[k]!r}, reference {ref!r}')
        assert isinstance(got[k], float)
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k])
        assert abs(got[k] - ref) <= MEAN_RTOL * abs(ref)
    assert call() == got                                                   # the same perm: bit-identical


def test_chamfer_scale_mat_and_generator():
    from poseprobe_amd import dtu_eval
    g = golden()
    s = np.diag([2.0, 2.0, 2.0, 1.0])
    s[:3, 3] = [1.0, -2.0, 0.5]
    args = (g['triangles'], g['stl'], g['obs_mask'], g['bb'], g['res'], g['plane'])
    a = dtu_eval.chamfer((g['vertices'].astype(np.float64) - s[:3, 3]) / 2.0, *args, runtime=True, perm=g['perm_rt'], scale_mat=s)
    b = dtu_eval.chamfer(torch.tensor(g['vertices']), *args, runtime=True, perm=torch.tensor(g['perm_rt']))
    assert [a[k] for k in COUNTS] == [b[k] for k in COUNTS] and abs(a['over_all'] - b['over_all']) < 1e-5
    gen = lambda: torch.Generator().manual_seed(11)
    c, d = (dtu_eval.chamfer(g['vertices'], *args, runtime=True, generator=gen()) for _ in range(2))
    assert c == d and c['n_sampled'] == b['n_sampled'] and abs(c['over_all'] - b['over_all']) < 0.05 * b['over_all']


def test_eval_on_files(tmp_path):
    sio = pytest.importorskip('scipy.io')
    from poseprobe_amd import dtu_eval, mesh
    g = golden()
    data = tmp_path / 'data'
    os.makedirs(data / 'ObsMask')
    os.makedirs(data / 'Points' / 'stl')
    mesh.write_ply(tmp_path / 'mesh.ply', g['vertices'], g['triangles'])
    mesh.write_ply(data / 'Points' / 'stl' / 'stl007_total.ply', g['stl'], np.empty((0, 3), np.int32))
    sio.savemat(data / 'ObsMask' / 'ObsMask7_10.mat', dict(ObsMask=g['obs_mask'], BB=g['bb'], Res=g['res']))
    sio.savemat(data / 'ObsMask' / 'Plane7.mat', dict(P=g['plane'].reshape(4, 1)))
    for tag, runtime in MODES:
        want = dtu_eval.chamfer(g['vertices'], g['triangles'], g['stl'], g['obs_mask'], g['bb'], g['res'], g['plane'], runtime=runtime,
                                perm=g[f'perm_{tag}'])
        got = dtu_eval.eval(tmp_path / 'mesh.ply', '7', tmp_path, dataset_dir=str(data), runtime=runtime, use_o3d=True,
                            perm=g[f'perm_{tag}'])
        assert got == tuple(want[k] for k in MEANS)
        assert (tmp_path / 'result.txt').read_text() == f'{got[0]} {got[1]} {got[2]}'
        for k, ref in zip(range(3), g[f'means_{tag}']):
            assert abs(got[k] - ref) <= MEAN_RTOL * abs(ref)
