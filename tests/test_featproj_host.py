"""CPU-only checks of the surface-projection feature pass: the float64 restatement against the reference's recorded run, the new
entry points' declarations, the trainer's gating and draws as functions of the step, and every refusal before the device is
touched."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import featproj_reference as R
from tests.helpers import load

NEW = ('pp_featproj_reproject', 'pp_featproj_loss')


def _queries(d):
    return ({k: torch.tensor(d[f'{t}.{k}']) for k in ('o', 'd', 't_min', 'acc')} for t in ('a', 'b'))


def _restated(d, dtype=torch.float64):
    qa, qb = _queries(d)
    i, j = (int(v) for v in d['pair'])
    feats = R.feature_maps('featproj_g24', R.NV, R.LAYERS)
    return R.restate(qa, qb, d['w2c'], R.intr_of(d['Ks']), i, j, float(d['nl']), float(d['voxel_size']), int(d['H']), int(d['W']), feats,
                     dtype=dtype)


def test_restatement_matches_the_recorded_loss():
    """Steps 3 to 7 in float64 on the recorded rays, entry distances and weighted step sums of both queries == the loss the
    reference's get_project_feature_loss returned, to the rounding of the reference's own float32 run (a mean of 44 cosines of
    float32 samples: 2e-6 relative is 16 ulp)."""
    d = load('featproj_g24.npz')
    out = _restated(d)
    print('loss', float(out['loss']), 'recorded', float(d['loss']), 'n_valid', out['n_valid'])
    assert abs(float(out['loss']) - float(d['loss'])) <= 2e-6 * abs(float(d['loss']))
    assert 16 <= out['n_valid'] < R.ROWS


def test_restatement_matches_the_recorded_flags_and_the_case_keeps_its_margins():
    d = load('featproj_g24.npz')
    qa, qb = _queries(d)
    i, j = (int(v) for v in d['pair'])
    for dtype in (torch.float64, torch.float32):                    # no row is a near-tie: either precision decides every row alike
        out = _restated(d, dtype)
        assert np.array_equal(out['valid'].numpy(), d['valid'])
    assert np.array_equal((qa['acc'] > 0).numpy(), d['hit']) and np.array_equal((qb['acc'] > 0).numpy(), d['hit_ref'])
    dec = R.decisions(qa, qb, d['w2c'], R.intr_of(d['Ks']), i, j, float(d['nl']), float(d['voxel_size']), int(d['H']), int(d['W']))
    assert R.decision_margin(dec, float(d['nl'])) > R.MARGIN
    # every geometric cause rejects some row of the recorded case, and some row survives them all
    assert all(int(v.sum()) > 0 for v in dec['reject'].values()), {k: int(v.sum()) for k, v in dec['reject'].items()}
    # the parameters the recorded run used are the ones the tests regenerate
    assert np.allclose(R.param_checksum(R.fixture_params()), d['P.checksum'], rtol=1e-12, atol=0)
    # step 2 restated == the rays query B was recorded with: they start at view j's centre and pass through the pixel
    pix = R.reproject(qa['o'], qa['d'], qa['t_min'], qa['acc'], d['w2c'], R.intr_of(d['Ks']), j, float(d['nl']))
    w2c = torch.tensor(d['w2c']).double()[j]
    K = torch.tensor(R.intr_of(d['Ks'])).double()[j]
    cam = qb['d'].double() @ w2c[:, :3].T
    assert torch.allclose(torch.stack([K[0] * cam[:, 0] / cam[:, 2] + K[2], K[1] * cam[:, 1] / cam[:, 2] + K[3]], -1), pix, rtol=1e-4, atol=1e-3)


def test_feature_generators_are_functions_of_the_case_name():
    a, b = R.feature_maps('x', 3, ((5, 4, 6), (1, 2, 2))), R.feature_maps('x', 3, ((5, 4, 6), (1, 2, 2)))
    assert [tuple(t.shape) for t in a] == [(3, 5, 4, 6), (3, 1, 2, 2)] and all(torch.equal(s, t) for s, t in zip(a, b))
    assert not torch.equal(a[0], R.feature_maps('y', 3, ((5, 4, 6),))[0])
    big = R.feature_maps('featproj_g24', R.NV, R.LAYERS)[0]
    assert big.dtype == torch.float32 and bool(torch.isfinite(big).all()) and 0.3 < float(big.std()) < 1.5


def test_new_entry_points_are_declared_and_the_abi_version_stays():
    from poseprobe_amd import _lib
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in NEW:
        assert name in protos, f'{name} is not declared in the header'
        fn = getattr(L, name)
        null = [0.0 if t is ctypes.c_float else (0 if t is ctypes.c_int32 else None) for t in fn.argtypes]
        assert fn(*null) == -1 and name.encode() in L.pp_last_error()       # null pointers are refused on the host
    assert _lib.header_abi_version() == 4 and L.pp_abi_version() == 4


# ---------------------------------------------------------------------------------------------------------------------------
def _stub_engine(**kw):
    d = dict(dev=torch.device('cpu'), se3_grad=torch.zeros(3, 6), deterministic=False, dist=None, featproj_rows=64, V=3, H=8, W=6,
             cfg=types.SimpleNamespace(N_iters=100), maps=[])
    d.update(kw)
    e = types.SimpleNamespace(**d)
    e.set_feature_maps = lambda f: e.maps.append(f)
    return e


def _trainer(engine=None, max_iter=40, **kw):
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.trainer import DualBranchTrainer
    sp = dict(features=['maps'], pairs=[(0, 1), (1, 2), (0, 2)], weight=1e-3, nl=0.05)
    sp.update(kw.pop('surface_projection', {}))
    return DualBranchTrainer(engine or _stub_engine(), bg_nerf.default_options(), max_iter=max_iter, surface_projection=sp, **kw)


def test_gating_is_the_object_phase_and_the_pose_phase():
    from poseprobe_amd.trainer import object_phase, pose_phase, surface_projection_active
    for step in range(0, 60):
        for n_obj, start in ((100, 0), (7, 0), (30, 5)):
            want = object_phase(step, n_obj, start) and pose_phase(step, 40, 0.3)
            assert surface_projection_active(step, 40, 0.3, n_obj, start) == want
    assert surface_projection_active(11, 40, 0.3, 100) and not surface_projection_active(12, 40, 0.3, 100)      # 40 * 0.3 = 12
    assert not surface_projection_active(8, 40, 0.3, 7) and not surface_projection_active(4, 40, 0.3, 30, 5)
    eng = _stub_engine(cfg=types.SimpleNamespace(N_iters=7))
    tr = _trainer(eng)
    assert eng.maps == [['maps']]                                        # the maps went to the engine once, at construction
    assert [tr._featproj_batch(s, 3) is not None for s in (0, 7, 8, 11, 12)] == [True, True, False, False, False]
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.trainer import DualBranchTrainer
    assert DualBranchTrainer(_stub_engine(), bg_nerf.default_options(), max_iter=10)._featproj_batch(0, 3) is None


def test_draw_sequence_is_a_function_of_the_seed_and_the_step_count():
    from poseprobe_amd.trainer import surface_projection_pair, surface_projection_sample_size
    pairs = [(0, 1), (1, 2), (0, 2)]
    assert surface_projection_sample_size(256, 8, 6) == 48 and surface_projection_sample_size(256, 400, 400) == 256
    rng = np.random.RandomState(5)
    assert surface_projection_pair(rng, pairs, 1) is None                       # no live pair: no draw
    assert surface_projection_pair(rng, pairs, 2) == (0, 1)
    twin = np.random.RandomState(5)
    twin.randint(1)
    assert [surface_projection_pair(rng, pairs, 3) for _ in range(6)] == [pairs[twin.randint(3)] for _ in range(6)]
    runs = []
    for _ in range(2):
        tr = _trainer(surface_projection=dict(seed=5, n_rays=20))
        seq = []
        for step in range(4):
            b = tr._featproj_batch(step, 2 if step < 2 else 3)
            r = b['rows']
            assert tr.last_featproj == dict(pair=(r['own'], r['other']), n_rows=20)
            assert r['src'].dtype == torch.int32 and r['src'].tolist() == [0] * 20 and r['pix'].shape == (20, 2)
            # pixel centres of distinct pixels of the 8 x 6 image
            x, y = r['pix'][:, 0] - 0.5, r['pix'][:, 1] - 0.5
            assert bool(((x == x.round()) & (y == y.round()) & (x >= 0) & (x < 6) & (y >= 0) & (y < 8)).all())
            assert len(set((y * 6 + x).tolist())) == 20
            assert (b['weight'], b['nl']) == (1e-3, 0.05)
            seq.append((tr.last_featproj['pair'], r['pix'].clone()))
        runs.append(seq)
    assert [p for p, _ in runs[0]][:2] == [(0, 1), (0, 1)]
    assert all(a[0] == b[0] and torch.equal(a[1], b[1]) for a, b in zip(*runs))
    assert not torch.equal(runs[0][0][1], runs[0][1][1])                       # a fresh pixel draw every step


def test_trainer_refusals():
    with pytest.raises(ValueError, match='featproj_rows >= 48'):
        _trainer(_stub_engine(featproj_rows=47))
    with pytest.raises(ValueError, match='deterministic=True'):
        _trainer(_stub_engine(deterministic=True))
    with pytest.raises(ValueError, match='deterministic=True'):
        _trainer(deterministic=True)


def test_joint_step_refusals_come_before_any_launch():
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.joint import DualBranchEngine
    net = lambda: bg_nerf.NeRF(bg_nerf.default_options(), device='cpu')
    fp = dict(rows={}, weight=1e-3, nl=0.05)
    with pytest.raises(ValueError, match='featproj is out of the scope of deterministic=True'):
        DualBranchEngine(_stub_engine(deterministic=True), net()).forward_backward(None, None, 0, None, None, featproj=fp)
    with pytest.raises(NotImplementedError, match='not sharded'):
        DualBranchEngine(_stub_engine(dist=object()), net()).forward_backward(None, None, 0, None, None, featproj=fp)


def test_engine_refusals_come_before_any_launch():
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    rs = syn.range_shape()
    mk = lambda **kw: TrainEngine(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, 8 ** 3, out_range=float(rs.max()), **kw.pop('cfg', {})),
                                  3, 8, 8, 16, device='cpu', **kw)
    rows = dict(src=torch.zeros(4, dtype=torch.int32), pix=torch.zeros(4, 2), own=1, other=2)
    plain = mk()
    assert plain.ws_featproj is None and plain.ws_featproj_ref is None and plain.featproj_rows == 0    # the default allocates nothing
    with pytest.raises(ValueError, match='featproj_rows > 0'):
        plain.surface_projection_grads(rows, 0, 1e-3, 0.05)
    with pytest.raises(NotImplementedError, match='inverse_y=True'):
        mk(featproj_rows=8, cfg=dict(inverse_y=False)).surface_projection_grads(rows, 0, 1e-3, 0.05)
    eng = mk(featproj_rows=8)
    assert eng.ws_featproj.N == 8 and eng.ws_featproj.cap == 8 * eng.cfg.n_samples
    # query B's workspace is forward-only: no activations kept, no gradient buffers
    assert eng.ws_featproj_ref.warp_acts is None and eng.ws_featproj_ref.rgb_acts is None and not hasattr(eng.ws_featproj_ref, 'g_alpha')
    with pytest.raises(ValueError, match='set_feature_maps'):
        eng.surface_projection_grads(rows, 0, 1e-3, 0.05)
    for bad, what in (([torch.zeros(2, 4, 3, 3)], 'n_views = 3'), ([torch.zeros(3, 513, 3, 3)], 'C <= 512'), ([torch.zeros(3, 4, 1, 3)], 'h, w >= 2'),
                      ([torch.zeros(3, 4, 3, 3)] * 5, '1 to 4'), ([], '1 to 4')):
        with pytest.raises(ValueError, match=what):
            eng.set_feature_maps(bad)
    eng.set_feature_maps([torch.arange(3 * 4 * 2 * 3, dtype=torch.float64).reshape(3, 4, 2, 3)])
    m = eng.feature_maps[0]
    assert m.shape == (3, 2, 3, 4) and m.dtype == torch.float32 and m.is_contiguous() and float(m[1, 1, 2, 3]) == float(24 + 3 * 6 + 5)
    with pytest.raises(ValueError, match='featproj_rows = 8'):
        eng.surface_projection_grads(dict(rows, src=torch.zeros(9, dtype=torch.int32)), 0, 1e-3, 0.05)
    with pytest.raises(ValueError, match=r'view pair \(1, 3\)'):
        eng.surface_projection_grads(dict(rows, other=3), 0, 1e-3, 0.05)
    eng.dist = object()
    with pytest.raises(NotImplementedError, match='not sharded'):
        eng.surface_projection_grads(rows, 0, 1e-3, 0.05)
    eng.dist, eng.deterministic = None, True
    with pytest.raises(ValueError, match='deterministic=True'):
        eng.surface_projection_grads(rows, 0, 1e-3, 0.05)
