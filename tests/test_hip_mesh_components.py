"""Connected components and the component filter on the GPU (poseprobe_amd.mesh.connected_components / keep_components,
csrc/pp_mesh_components.hip) against the numpy restatement of their semantics (tests/mesh_components_reference.py, itself checked
against scipy in tests/test_mesh_components_host.py).  Everything compared is an integer or a copied float: torch.equal, no
tolerance.  The number of rounds is compared too - the kernels' schedule makes it a pure function of the mesh."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import mesh_components_reference as R
from tests import mesh_reference as M
from tests.helpers import load

pytestmark = pytest.mark.gpu

MESHES = ('three_body', 'noise', 'big_and_small')
STRIPS = ('ascending', 'descending', 'random')
CASES = sorted(R.small_cases()) + list(MESHES) + ['strip_' + s for s in STRIPS]


@functools.lru_cache(maxsize=None)
def case(name):
    """(vertices [Nv,3] float32, triangles [Nt,3] int32, restated components, restated rounds) - computed once, read-only."""
    if name in MESHES:
        v, t = R.mc_mesh(name)
    else:
        t, nv = R.strip(R.STRIP_TRIANGLES, name[6:]) if name.startswith('strip_') else R.small_cases()[name]
        v = np.random.RandomState(7).rand(nv, 3).astype(np.float32)
    v.setflags(write=False)
    t.setflags(write=False)
    return v, t, R.connected_components(t, len(v)), R.rounds(t, len(v))[1]


def dev(a, dtype=None):
    return torch.from_numpy(np.array(a)).to(device='cuda', dtype=dtype)           # (a copy: the cases are read-only)


def same(got, want):
    """torch.equal of a device tensor and a numpy array, dtype and shape included."""
    want = torch.from_numpy(np.array(want))
    return got.is_cuda and got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.cpu(), want)


def check_components(got, want):
    for key in ('labels', 'roots', 'vertex_counts', 'triangle_counts'):
        assert same(got[key], want[key]), key
    assert got['n_components'] == want['n_components'] and isinstance(got['n_components'], int)


def check_kept(got, want, attributes=()):
    for key in ('vertices', 'triangles', 'vertex_index') + tuple(attributes):
        assert same(got[key], want[key]), key
    assert (got['n_components'], got['n_kept']) == (want['n_components'], want['n_kept'])


# ---- 1. index by index ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', CASES)
def test_components_and_filter_equal_the_restatement(name):
    from poseprobe_amd import mesh
    v, t, want, want_rounds = case(name)
    info = {}
    got = mesh.connected_components(dev(t), len(v), info)
    check_components(got, want)
    print(f'{name}: {len(v)} vertices, {len(t)} triangles, {got["n_components"]} components, {info["rounds"]} rounds '
          f'(restated schedule: {want_rounds})')
    assert info['rounds'] == want_rounds
    if name.startswith('strip_'):
        assert info['rounds'] > mesh.CC_BATCH               # more than one batch: the host loop went round and read its flags twice
        assert got['n_components'] == 1 and int(got['labels'].max()) == 0
    check_components(mesh.connected_components(t, len(v)), want)          # a numpy array is uploaded
    info = {}
    check_kept(mesh.keep_components(dev(v), dev(t), 'largest', info=info), R.keep_components(v, t, 'largest'))
    assert info['rounds'] == want_rounds


def test_three_bodies_and_noise():
    from poseprobe_amd import mesh
    v, t, _, _ = case('three_body')
    got = mesh.connected_components(dev(t), len(v))
    cc = {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in got.items()}
    assert cc['n_components'] == 3
    euler = []
    for root in cc['roots']:
        sub, n = R.component_mesh(cc, t, root)
        assert M.is_closed_manifold(sub, n)
        euler.append((M.euler_characteristic(sub, n), bool(v[cc['labels'] == root][:, 2].mean() < 9)))
    assert sorted(euler) == [(0, True), (2, False), (2, False)]           # the torus lies in the low z layers
    assert mesh.connected_components(dev(case('noise')[1]), len(case('noise')[0]))['n_components'] == case('noise')[2]['n_components'] > 100


# ---- 2. relabelling -------------------------------------------------------------------------------------------------------------------
def test_a_permuted_numbering_gives_the_same_partition():
    from poseprobe_amd import mesh
    v, t, want, _ = case('noise')
    perm = np.random.RandomState(11).permutation(len(v)).astype(np.int32)            # old index -> new index
    got = mesh.connected_components(dev(perm[t]), len(v))
    lab = got['labels'].cpu().numpy()
    assert got['n_components'] == want['n_components']
    old = want['labels']
    referenced = old >= 0
    assert ((lab[perm] >= 0) == referenced).all()
    # the same partition: one new label per old label and the other way round
    pairs = np.unique(np.stack([old[referenced], lab[perm][referenced]], -1), axis=0)
    assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])) == want['n_components']
    # and the label is the smallest NEW index of the part
    smallest = np.full(len(v), len(v), dtype=np.int64)
    np.minimum.at(smallest, old[referenced], perm[referenced])
    assert np.array_equal(lab[perm][referenced], smallest[old[referenced]])
    check_components(got, R.connected_components(perm[t], len(v)))


# ---- 3. the filter keeps exactly the object -------------------------------------------------------------------------------------------
def test_largest_component_of_two_spheres_is_the_mesh_of_the_big_one():
    from poseprobe_amd import mesh
    vb, tb = mesh.marching_cubes(R.big_field(), 0.0)
    assert same(vb, R.mc_mesh('big')[0]) and same(tb, R.mc_mesh('big')[1])
    v, t = mesh.marching_cubes(R.big_and_small_field(), 0.0)
    assert len(v) > len(vb)
    k = mesh.keep_components(v, t, keep='largest')
    assert torch.equal(k['vertices'], vb) and torch.equal(k['triangles'], tb)
    assert k['n_components'] == 2 and k['n_kept'] == 1 and torch.equal(v[k['vertex_index'].long()], vb)


@pytest.mark.parametrize('keep', [8, 0, 10 ** 9, 0.5, 0.0002, 0.99])
def test_count_and_fraction_rules_with_attributes(keep):
    from poseprobe_amd import mesh
    v, t, _, _ = case('noise')
    rs = np.random.RandomState(5)
    attributes = dict(colors=rs.rand(len(v), 3).astype(np.float32), ids=np.arange(len(v), dtype=np.int64), m=rs.rand(len(v), 2, 2))
    want = R.keep_components(v, t, keep, attributes)
    got = mesh.keep_components(dev(v), dev(t), keep, attributes={k: dev(a) for k, a in attributes.items()})
    check_kept(got, want, attributes)
    print(f'keep={keep}: {got["n_kept"]} of {got["n_components"]} components, {len(got["vertices"])} of {len(v)} vertices')
    assert same(got['ids'].to(torch.int32), want['vertex_index'])
    mixed = mesh.keep_components(v, t, keep, attributes=dict(colors=attributes['colors']))          # numpy in: numpy rows out
    assert isinstance(mixed['colors'], np.ndarray) and np.array_equal(mixed['colors'], want['colors'])


# ---- 4. two runs, the same bits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['noise', 'strip_random'])
def test_two_runs_give_the_same_bits(name):
    from poseprobe_amd import mesh
    v, t, _, _ = case(name)
    dv, dt = dev(v), dev(t)
    runs = []
    for _ in range(2):
        info = {}
        cc = mesh.connected_components(dt, len(v), info)
        k = mesh.keep_components(dv, dt, 4, attributes=dict(a=dv[:, 0].clone()))
        runs.append((cc, k, info['rounds']))
    (cc0, k0, r0), (cc1, k1, r1) = runs
    assert r0 == r1 and cc0['labels'].data_ptr() != cc1['labels'].data_ptr()
    for a, b in ((cc0, cc1), (k0, k1)):
        assert set(a) == set(b)
        for key in a:
            assert torch.equal(a[key], b[key]) if isinstance(a[key], torch.Tensor) else a[key] == b[key], key


# ---- 5. bounds ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['unreferenced', 'one_triangle', 'noise', 'strip_random'])
def test_kernels_stay_inside_their_buffers(name):
    """labels, the workspace, the flags, the counts, the masks and the compacted outputs sit between guard words; row counts that
    are no multiple of the 256-thread work-group (16 / 4, 3 / 1, 19955 / 39388, 4098 / 4096).  Run once per case."""
    from poseprobe_amd import mesh, ops
    v, t, want, want_rounds = case(name)
    Nv, Nt = len(v), len(t)
    assert Nv % 256 != 0
    PAD, SENT = 4096, 0x7FC0DEAD
    fences = {}

    def fenced(what, n, dtype=torch.int32):
        words = (n * torch.empty(0, dtype=dtype).element_size() + 3) // 4
        arena = torch.full((words + 2 * PAD,), SENT, dtype=torch.int32, device='cuda')
        fences[what] = (arena, words)
        return arena[PAD:PAD + words].view(dtype)[:n]

    dv, dt = dev(v), dev(t)
    labels, work, changed = fenced('labels', Nv), fenced('work', ops.cc_workspace(Nv), torch.uint8), fenced('changed', want_rounds)
    ops.cc_rounds(dt, Nv, 0, want_rounds, labels, work, changed)
    assert changed.tolist() == [1] * (want_rounds - 1) + [0]
    by_v, by_t = fenced('vertex_counts', Nv), fenced('triangle_counts', Nv)
    ops.cc_count(labels, dt, by_v, by_t)
    root_keep = torch.zeros(Nv, dtype=torch.uint8, device='cuda')
    big = want['roots'][np.argmax(want['triangle_counts'])]
    root_keep[int(big)] = 1
    vkeep, tkeep = fenced('vertex_keep', Nv), fenced('triangle_keep', Nt)
    ops.cc_keep_masks(labels, dt, root_keep, vkeep, tkeep)
    ref = R.keep_components(v, t, 'largest')
    nv, nt = len(ref['vertices']), len(ref['triangles'])
    assert (int(vkeep.sum()), int(tkeep.sum())) == (nv, nt)
    out_v = fenced('out_vertices', nv * 3, torch.float32).view(nv, 3)
    out_i, out_t = fenced('out_index', nv), fenced('out_triangles', nt * 3).view(nt, 3)
    ops.cc_compact(dv, dt, torch.cumsum(vkeep, 0, dtype=torch.int32), torch.cumsum(tkeep, 0, dtype=torch.int32), out_v, out_i, out_t)
    torch.cuda.synchronize()
    for what, (arena, words) in fences.items():
        assert bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + words:] == SENT).all()), what
    assert same(labels, want['labels']) and same(by_v[dev(want['roots']).long()], want['vertex_counts'])
    assert same(by_t[dev(want['roots']).long()], want['triangle_counts']) and int(by_v.sum()) == int((want['labels'] >= 0).sum())
    assert same(out_v, ref['vertices']) and same(out_i, ref['vertex_index']) and same(out_t, ref['triangles'])
    # fewer output rows than kept rows: the rows past the end are not written
    if nv > 1 and nt > 1:
        short_v, short_i = fenced('short_vertices', (nv - 1) * 3, torch.float32).view(nv - 1, 3), fenced('short_index', nv - 1)
        short_t = fenced('short_triangles', (nt - 1) * 3).view(nt - 1, 3)
        ops.cc_compact(dv, dt, torch.cumsum(vkeep, 0, dtype=torch.int32), torch.cumsum(tkeep, 0, dtype=torch.int32), short_v, short_i, short_t)
        torch.cuda.synchronize()
        for what in ('short_vertices', 'short_index', 'short_triangles'):
            arena, words = fences[what]
            assert bool((arena[:PAD] == SENT).all()) and bool((arena[PAD + words:] == SENT).all()), what
        assert same(short_v, ref['vertices'][:-1]) and same(short_t, ref['triangles'][:-1])


# ---- 6. the round cap -----------------------------------------------------------------------------------------------------------------
def test_round_cap_raises_and_launches_nothing_more(monkeypatch):
    from poseprobe_amd import mesh, ops
    v, t, _, want_rounds = case('strip_descending')
    assert want_rounds > mesh.CC_BATCH
    calls = []
    for fn in ('cc_rounds', 'cc_count', 'cc_keep_masks', 'cc_compact'):
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _real=real, _fn=fn: (calls.append(_fn), _real(*a))[1])
    monkeypatch.setattr(mesh, 'CC_MAX_BATCHES', 1)
    with pytest.raises(RuntimeError, match=rf'after {mesh.CC_BATCH} rounds'):
        mesh.keep_components(dev(v), dev(t), 'largest')
    assert calls == ['cc_rounds']
    calls.clear()
    monkeypatch.setattr(mesh, 'CC_MAX_BATCHES', -(-want_rounds // mesh.CC_BATCH))        # just enough
    assert mesh.connected_components(dev(t), len(v))['n_components'] == 1
    assert calls == ['cc_rounds'] * -(-want_rounds // mesh.CC_BATCH) + ['cc_count']


def test_the_filter_checks_the_indices_once(monkeypatch):
    """keep_components hands connected_components the triangles it has checked: one aminmax and one host read for the range."""
    from poseprobe_amd import mesh
    v, t, _, _ = case('big_and_small')
    calls = []
    real = torch.aminmax
    monkeypatch.setattr(torch, 'aminmax', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert mesh.keep_components(dev(v), dev(t), 'largest')['n_kept'] == 1
    assert len(calls) == 1
    del calls[:]
    assert mesh.connected_components(dev(t), len(v))['n_components'] == 2
    assert len(calls) == 1


# ---- 7. drivers -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def model():
    """The 24^3 drop-in model of the forward fixtures with a floater: its own mesh is one component, so a block of 3^3 template
    nodes in a corner of the box, where the template is positive (outside), is set to -0.5 (inside)."""
    from tests.test_hip_dropin import make_model
    m = make_model(load('inference_g24.npz')).eval()
    with torch.no_grad():
        corner = m.sdf.grid[0, 0, 2:5, 2:5, 2:5]
        assert float(corner.min()) > 0
        corner.fill_(-0.5)
    return m


def test_validate_deform_mesh_keeps_the_largest_component(tmp_path):
    from poseprobe_amd import dtu_eval, mesh
    m = model()
    m.progress.data.fill_(1.0)
    cfg = types.SimpleNamespace(basedir=str(tmp_path), expname='g24')
    path = lambda prefix: os.path.join(str(tmp_path), 'g24', 'meshes', 'deform' + prefix + '.ply')
    assert dtu_eval.validate_deform_mesh(m, cfg, resolution=24, extract_color=True, prefix='_all') == 0.0
    assert dtu_eval.validate_deform_mesh(m, cfg, resolution=24, extract_color=True, prefix='_none', keep=None) == 0.0
    assert open(path('_all'), 'rb').read() == open(path('_none'), 'rb').read()
    assert dtu_eval.validate_deform_mesh(m, cfg, resolution=24, extract_color=True, prefix='_kept', keep='largest') == 0.0
    a, k = mesh.read_ply_attributes(path('_all')), mesh.read_ply_attributes(path('_kept'))
    want = R.keep_components(a['vertices'], a['triangles'], 'largest')
    print(f'fixture model at 24^3: {want["n_components"]} components, {len(k["vertices"])} of {len(a["vertices"])} vertices kept')
    assert want['n_components'] >= 2 and 0 < len(k['vertices']) < len(a['vertices'])
    assert len(k['triangles']) > 0 and mesh.connected_components(k['triangles'], len(k['vertices']))['n_components'] == 1
    assert np.array_equal(k['vertices'], want['vertices']) and np.array_equal(k['triangles'], want['triangles'])
    assert k['colors'].dtype == np.uint8 and np.array_equal(k['colors'], a['colors'][want['vertex_index']])
    # the plain driver
    dtu_eval.validate_mesh(m, cfg, resolution=24, prefix='all')
    dtu_eval.validate_mesh(m, cfg, resolution=24, prefix='none', keep=None)
    dtu_eval.validate_mesh(m, cfg, resolution=24, prefix='kept', keep='largest')
    plain = lambda prefix: os.path.join(str(tmp_path), 'g24', 'meshes', '122_' + prefix + '.ply')
    assert open(plain('all'), 'rb').read() == open(plain('none'), 'rb').read()
    a, k = mesh.read_ply(plain('all')), mesh.read_ply(plain('kept'))
    want = R.keep_components(a[0], a[1], 'largest')
    assert want['n_components'] >= 2 and len(k[0]) < len(a[0])
    assert np.array_equal(k[0], want['vertices']) and np.array_equal(k[1], want['triangles']) and len(k[1]) > 0
