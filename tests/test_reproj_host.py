"""CPU-only checks of the engine-native reprojection pass: the new entry points are declared and validate their arguments on
the host, the trainer draws its pair / mode / rows as documented, and every refusal happens before the device is touched."""
import ctypes
import types

import numpy as np
import pytest
import torch

NEW = ('pp_reproj_rays', 'pp_reproj_dense_pts', 'pp_reproj_loss', 'pp_reproj_pose_fold')


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


def _stub_engine(**kw):
    d = dict(dev=torch.device('cpu'), se3_grad=torch.zeros(3, 6), deterministic=False, dist=None, reproj_rows=64, V=3,
             cfg=types.SimpleNamespace(N_iters=100))
    d.update(kw)
    return types.SimpleNamespace(**d)


def _pairs(P=(10, 50, 7)):
    g = torch.Generator().manual_seed(0)
    mk = lambda n: (torch.rand(n, 2, generator=g) * 31, torch.rand(n, 2, generator=g) * 31, torch.rand(n, generator=g))
    return [(0, 1, *mk(P[0])), (1, 2, *mk(P[1])), (0, 2, *mk(P[2]))]


def _trainer(engine=None, **kw):
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.trainer import DualBranchTrainer
    opt = bg_nerf.default_options()
    rp = dict(pairs=_pairs(), nl=0.05, weight_projection=1e-3, weight_near_surface=1e-1)
    rp.update(kw.pop('reprojection', {}))
    return DualBranchTrainer(engine or _stub_engine(), opt, max_iter=10, reprojection=rp, **kw)


def test_trainer_draws_one_live_pair_and_switches_the_mode_with_the_third_view():
    from poseprobe_amd.trainer import reproj_sample_size
    tr = _trainer(reprojection=dict(seed=3))
    rng = np.random.RandomState(3)
    pairs = _pairs()
    # two active views: only the pair (0, 1) is live, the surface point is the zero crossing of the template
    b = tr._reproj_batch(5, 2)
    rng.randint(1)
    assert tr.last_reproj == dict(pair=(0, 1), mode='crossing', n_rows=20) and b['mode'] == 'crossing'
    r = b['rows']
    assert r['own'].dtype == torch.int32 and r['own'].tolist() == [1] * 10 + [0] * 10 and r['other'].tolist() == [0] * 10 + [1] * 10
    assert torch.equal(r['pix'], torch.cat([pairs[0][3], pairs[0][2]])) and torch.equal(r['match'], torch.cat([pairs[0][2], pairs[0][3]]))
    assert torch.equal(r['conf'], torch.cat([pairs[0][4]] * 2))
    assert (b['weight_projection'], b['weight_near_surface'], b['nl'], b['pixel_thre']) == (1e-3, 1e-1, 0.05, 200)
    # three active views: every pair is live, drawn as RandomState(seed).randint does; the rendered depth gives the point
    seen = set()
    for step in range(12):
        b = tr._reproj_batch(step, 3)
        i, j = pairs[rng.randint(3)][:2]
        assert tr.last_reproj['pair'] == (i, j) and b['mode'] == 'render'
        n = reproj_sample_size({(0, 1): 10, (1, 2): 50, (0, 2): 7}[(i, j)], 64)
        assert b['rows']['own'].shape[0] == 2 * n == tr.last_reproj['n_rows']
        seen.add((i, j))
    assert len(seen) == 3


def test_matches_beyond_half_the_row_capacity_are_subsampled_without_repetition():
    from poseprobe_amd.trainer import reproj_sample_size
    assert [reproj_sample_size(n, 64) for n in (1, 32, 33, 500)] == [1, 32, 32, 32]
    tr = _trainer(reprojection=dict(pairs=_pairs()[1:2]))
    ci, cj, conf = _pairs()[1][2:]
    picks = []
    for step in range(2):
        r = tr._reproj_batch(step, 3)['rows']
        assert r['own'].shape[0] == 64 and r['pix'].shape == (64, 2)
        # rows [0, 32) are matches seen from view j, rows [32, 64) the same matches from view i
        idx = [int((ci == m).all(dim=1).nonzero()[0, 0]) for m in r['match'][:32]]
        assert len(set(idx)) == 32
        assert torch.equal(r['pix'][:32], cj[idx]) and torch.equal(r['pix'][32:], ci[idx]) and torch.equal(r['conf'][32:], conf[idx])
        picks.append(idx)
    assert picks[0] != picks[1]                                  # a fresh subset every step


def test_term_is_active_in_the_object_phase_only():
    tr = _trainer(_stub_engine(cfg=types.SimpleNamespace(N_iters=7)))
    assert tr._reproj_batch(7, 3) is not None and tr._reproj_batch(8, 3) is None
    tr = _trainer(reprojection=dict(n_iters_object=50, start_object=4))
    assert tr._reproj_batch(3, 3) is None and tr._reproj_batch(4, 3) is not None and tr._reproj_batch(51, 3) is None
    # no live pair (the second view of every pair is not in play yet): no term
    assert _trainer(reprojection=dict(pairs=_pairs()[1:]))._reproj_batch(0, 2) is None
    from poseprobe_amd.trainer import DualBranchTrainer
    from poseprobe_amd import bg_nerf
    assert DualBranchTrainer(_stub_engine(), bg_nerf.default_options(), max_iter=10)._reproj_batch(0, 3) is None


def test_an_empty_pair_takes_part_in_the_draw():
    pairs = _pairs()
    empty = (0, 2, torch.zeros(0, 2), torch.zeros(0, 2), torch.zeros(0))
    tr = _trainer(reprojection=dict(pairs=pairs[:2] + [empty], seed=5))
    rng = np.random.RandomState(5)
    got_none = 0
    for step in range(20):
        b = tr._reproj_batch(step, 3)
        k = rng.randint(3)                                           # the draw is over ALL live pairs, the empty one included
        if k == 2:
            assert b is None
            got_none += 1
        else:
            assert tr.last_reproj['pair'] == pairs[k][:2]
    assert got_none > 0


def test_a_box_without_a_finite_diagonal_is_refused():
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    cfg = SceneConfig([-2., -2., -2.], [1., 1., 1.], 8 ** 3)            # sum(xyz_max - xyz_min ** 2) = -9: the (sic) formula gives NaN
    with pytest.raises(ValueError, match='diagonal_length is not finite'):
        TrainEngine(cfg, 3, 8, 8, 16, device='cpu', reproj_rows=8)
    assert TrainEngine(cfg, 3, 8, 8, 16, device='cpu').ws_reproj is None


def test_trainer_refusals():
    with pytest.raises(ValueError, match='reproj_rows'):
        _trainer(_stub_engine(reproj_rows=0))
    with pytest.raises(ValueError, match='deterministic=True'):
        _trainer(_stub_engine(deterministic=True))


def test_joint_step_refusals_come_before_any_launch():
    from poseprobe_amd import bg_nerf
    from poseprobe_amd.joint import DualBranchEngine
    net = lambda: bg_nerf.NeRF(bg_nerf.default_options(), device='cpu')
    rp = dict(rows={}, mode='render', weight_projection=1., weight_near_surface=1., nl=0.05, pixel_thre=200)
    with pytest.raises(ValueError, match='deterministic=True'):
        DualBranchEngine(_stub_engine(deterministic=True), net()).forward_backward(None, None, 0, None, None, reproj=rp)
    with pytest.raises(NotImplementedError, match='not sharded'):
        DualBranchEngine(_stub_engine(dist=object()), net()).forward_backward(None, None, 0, None, None, reproj=rp)


def test_engine_refusals_come_before_any_launch():
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    rs = syn.range_shape()
    mk = lambda **kw: TrainEngine(SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, 8 ** 3, out_range=float(rs.max()), **kw.pop('cfg', {})),
                                  3, 8, 8, 16, device='cpu', **kw)
    rows = dict(own=torch.zeros(4, dtype=torch.int32))
    plain = mk()
    assert plain.ws_reproj is None and plain.reproj_rows == 0       # the default allocates nothing
    with pytest.raises(ValueError, match='reproj_rows > 0'):
        plain.reprojection_grads(rows, 'render', 0)
    with pytest.raises(NotImplementedError, match='inverse_y=True'):
        mk(reproj_rows=8, cfg=dict(inverse_y=False)).reprojection_grads(rows, 'render', 0)
    eng = mk(reproj_rows=8)
    assert eng.ws_reproj.N == 8 and eng.ws_reproj.cap == 8 * eng.cfg.n_samples
    with pytest.raises(ValueError, match="'crossing' or 'render'"):
        eng.reprojection_grads(rows, 'depth', 0)
    with pytest.raises(ValueError, match='reproj_rows = 8'):
        eng.reprojection_grads(dict(own=torch.zeros(9, dtype=torch.int32)), 'render', 0)
    eng.dist = object()
    with pytest.raises(NotImplementedError, match='not sharded'):
        eng.reprojection_grads(rows, 'render', 0)


def test_the_autograd_pose_term_route_is_gone():
    """trainer.ReprojectionTerm, DualBranchTrainer(pose_terms=) and DualBranchEngine.train_step(before_step=) were the autograd route
    of the pose terms; reprojection= / surface_projection= on the engine's own launches are the only one."""
    from poseprobe_amd import bg_nerf, trainer
    from poseprobe_amd.joint import DualBranchEngine
    assert not hasattr(trainer, 'ReprojectionTerm')
    with pytest.raises(TypeError, match='pose_terms'):
        trainer.DualBranchTrainer(_stub_engine(), bg_nerf.default_options(), max_iter=10, pose_terms=())
    joint = DualBranchEngine(_stub_engine(), bg_nerf.NeRF(bg_nerf.default_options(), device='cpu'))
    with pytest.raises(TypeError, match='before_step'):
        joint.train_step(None, None, 0, None, None, before_step=lambda: None)
