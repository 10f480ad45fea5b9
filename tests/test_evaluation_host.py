"""CPU checks of poseprobe_amd.evaluation: the SSIM restatement of tests/evaluation_reference.py against the
recorded reference (tests/golden/eval_metrics.npz, tools/make_eval_golden.py), the pose functions against the recorded outputs
of the reference's own and against known Sim(3) moves, and the argument checks of pp_ssim through ctypes (no GPU call)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import evaluation_reference as R
from tests.helpers import load

# Largest difference between the float32 and the float64 run of the reference's own functions on the fixture's pose cases
# (printed by tools/make_eval_golden.py), per quantity; the tolerance is 4 x that, for the order of operations.
SPREAD = dict(angle=1.730e-07, R=2.353e-03, t=7.627e-05, aligned=9.019e-07, backtrack=5.221e-07, sim3_R=7.451e-08, sim3_s=2.679e-07,
              sim3_t=3.012e-07)
TOL = {k: 4 * v for k, v in SPREAD.items()}
R_FLOOR = float(np.degrees(np.arccos(1 - 1e-7)))       # rotation_distance of identical rotations: its clamp keeps it there


@pytest.fixture(scope='module')
def golden():
    return load('eval_metrics.npz')


def test_the_fixture_was_recorded_for_the_kernels_tile(golden):
    from poseprobe_amd import ops
    assert int(golden['tile']) == R.GOLDEN_T == ops.ssim_tile()


def test_ssim_restatement_equals_the_recorded_reference(golden):
    n = 0
    for case in R.ssim_cases(int(golden['tile'])):
        for i, (x, y) in enumerate(case['pairs']):
            key = f'ssim.{case["name"]}.{i}'
            m = R.rgb_ssim(x, y, case['max_val'], filter_size=case['fs'], return_map=True)
            assert m.shape == golden[key + '.map'].shape == (x.shape[0] - case['fs'] + 1, x.shape[1] - case['fs'] + 1, 3)
            assert np.abs(m - golden[key + '.map']).max() <= 1e-12, key
            assert abs(R.rgb_ssim(x, y, case['max_val'], filter_size=case['fs']) - golden[key + '.value']) <= 1e-12, key
            n += 1
    assert n == 15
    assert abs(golden['ssim.zeros_ones.0.value'] - 9.999e-5) < 1e-8
    assert golden['ssim.negated.0.value'] < -0.9 and golden['ssim.identical.0.value'] == 1.0


def _t(x, dtype=torch.float32):
    return torch.tensor(x, dtype=dtype)


@pytest.mark.parametrize('name', ['B3', 'B9', 'B10', 'B25'])
def test_pose_functions_match_the_recorded_reference(golden, name):
    from poseprobe_amd import evaluation as E
    case = {c['name']: c for c in R.pose_cases()}[name]
    pose, GT = _t(case['pose']), _t(case['GT'])
    g = lambda k: golden[f'pose.{name}.{k}']

    def close(got, key, q):
        got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, np.float64)
        d = np.abs(got - g(key)).max()
        print(f'{name} {key}: off by {d:.3e} (tolerance {TOL[q]:.3e})')
        assert got.shape == g(key).shape and d <= TOL[q], (key, d)

    c2w, c2w_GT = E._invert(pose), E._invert(GT)
    close(E.rotation_distance(c2w[..., :3], c2w_GT[..., :3]), 'rotation_distance.angle', 'angle')
    e = E.evaluate_camera_alignment(pose, GT)
    close(e.R, 'unaligned.R', 'R'), close(e.t, 'unaligned.t', 't')
    for tag, fn in (('small', E.prealign_w2c_small_camera_systems), ('large', E.prealign_w2c_large_camera_systems)):
        aligned, sim3 = fn(pose, GT)
        assert sim3.type == 'traj_align' and sim3.R.shape == (1, 3, 3) and sim3.t.shape == (1, 3, 1) and aligned.dtype == torch.float32
        close(aligned, f'{tag}.aligned', 'aligned')
        close(sim3.R, f'{tag}.sim3_R', 'sim3_R'), close(sim3.t, f'{tag}.sim3_t', 'sim3_t')
        close(torch.as_tensor(sim3.s), f'{tag}.sim3_s', 'sim3_s')
        e = E.evaluate_camera_alignment(aligned, GT)
        close(e.R, f'{tag}.R', 'R'), close(e.t, f'{tag}.t', 't')
        close(E.backtrack_from_aligning_the_trajectory(GT, sim3), f'{tag}.backtrack', 'backtrack')
    error, aligned, sim3 = E.evaluate_poses(pose, GT)
    tag = 'large' if len(pose) > 9 else 'small'
    close(aligned, f'{tag}.aligned', 'aligned'), close(error.R, f'{tag}.R', 'R'), close(error.t, f'{tag}.t', 't')


@pytest.mark.parametrize('B', [3, 9, 10, 25])
def test_both_aligners_undo_a_known_sim3(B):
    """Ground truth moved by a Sim(3) with s = 1.7: either aligner recovers it, the error falls to zero - for the rotation to
    acos(1 - eps), where rotation_distance's clamp keeps it - and backtrack carries the ground truth onto the moved poses.  In
    float64 (the functions keep the dtype): next to its floor the float32 angle moves in steps of 0.006 degrees, which the
    tolerance measured at errors of 2 degrees does not describe."""
    from poseprobe_amd import evaluation as E
    GT = R.ground_truth_poses(B)
    s, Rm, t = R.known_sim3()
    moved = R.move_by_sim3(GT, s, Rm, t)
    for fn in (E.prealign_w2c_small_camera_systems, E.prealign_w2c_large_camera_systems):
        aligned, sim3 = fn(_t(moved, torch.float64), _t(GT, torch.float64))
        e = E.evaluate_camera_alignment(aligned, _t(GT, torch.float64))
        assert aligned.dtype == torch.float64
        assert (e.R - R_FLOOR).abs().max() <= TOL['R'] and e.t.max() <= TOL['t'], (fn.__name__, e)
        assert abs(float(sim3.s) - s) <= TOL['sim3_s'] * s
        assert np.abs(sim3.R[0].numpy() - Rm).max() <= TOL['sim3_R'] and np.abs(sim3.t[0, :, 0].numpy() - t).max() <= TOL['sim3_t'] * s
        back = E.backtrack_from_aligning_the_trajectory(_t(GT, torch.float64), sim3)
        assert np.abs(back.numpy() - moved).max() <= TOL['backtrack']
    error, aligned, sim3 = E.evaluate_poses(_t(moved, torch.float64), _t(GT, torch.float64))
    assert (error.R - R_FLOOR).abs().max() <= TOL['R'] and error.t.max() <= TOL['t']


def test_the_pair_search_avoids_a_perturbed_anchor_and_stops_at_ten_poses():
    from poseprobe_amd import evaluation as E
    GT = R.ground_truth_poses(5)
    moved = R.move_by_sim3(GT, *R.known_sim3())
    for bad in range(5):
        pose = R.perturb(moved, 20.0, 0.5, seed=bad, only=(bad,))
        aligned, sim3 = E.prealign_w2c_small_camera_systems(_t(pose, torch.float64), _t(GT, torch.float64))
        e = E.evaluate_camera_alignment(aligned, _t(GT, torch.float64))
        good = [i for i in range(5) if i != bad]
        # anchored at a good pose, with a good partner for the scale, every good pose aligns exactly
        assert (e.R[good] - R_FLOOR).abs().max() <= TOL['R'] and e.t[good].max() <= TOL['t'], (bad, e)
        assert e.R[bad] > 5
    # only the first ten poses are candidates: with all of them perturbed and the rest exact, no candidate aligns exactly
    GT = R.ground_truth_poses(12)
    moved = R.move_by_sim3(GT, *R.known_sim3())
    pose = R.perturb(moved, 20.0, 0.5, seed=9, only=tuple(range(10)))
    aligned, _ = E.prealign_w2c_small_camera_systems(_t(pose, torch.float64), _t(GT, torch.float64))
    assert E.evaluate_camera_alignment(aligned, _t(GT, torch.float64)).t[10:].min() > 1.0


def test_evaluate_poses_switches_aligner_above_nine_poses(monkeypatch):
    from poseprobe_amd import evaluation as E
    used = []
    small, large = E.prealign_w2c_small_camera_systems, E.prealign_w2c_large_camera_systems
    monkeypatch.setattr(E, 'prealign_w2c_small_camera_systems', lambda *a: used.append('small') or small(*a))
    monkeypatch.setattr(E, 'prealign_w2c_large_camera_systems', lambda *a: used.append('large') or large(*a))
    for B in (2, 9, 10, 25):
        GT = R.ground_truth_poses(B)
        E.evaluate_poses(_t(R.move_by_sim3(GT, *R.known_sim3())), _t(GT))
    assert used == ['small', 'small', 'large', 'large']


def test_a_single_pose_and_mismatched_shapes_are_refused():
    from poseprobe_amd import evaluation as E
    GT = _t(R.ground_truth_poses(3))
    with pytest.raises(ValueError):
        E.prealign_w2c_small_camera_systems(GT[:1], GT[:1])
    with pytest.raises(ValueError):
        E.evaluate_poses(GT[:1], GT[:1])
    with pytest.raises(ValueError):
        E.prealign_w2c_small_camera_systems(GT, GT[:2])
    with pytest.raises(ValueError):
        E.prealign_w2c_large_camera_systems(GT, GT[:2])


def test_the_trajectory_alignment_falls_back_to_the_identity(monkeypatch):
    from poseprobe_amd import evaluation as E

    def fail(*a, **k):
        raise np.linalg.LinAlgError('SVD did not converge')

    monkeypatch.setattr(np.linalg, 'svd', fail)
    pose, GT = _t(R.ground_truth_poses(11, seed=1)), _t(R.ground_truth_poses(11))
    aligned, sim3 = E.prealign_w2c_large_camera_systems(pose, GT)
    assert sim3.s == 1. and torch.equal(sim3.R[0], torch.eye(3)) and not sim3.t.any() and sim3.type == 'traj_align'
    assert (aligned - pose).abs().max() <= 1e-6


def test_rgb_ssim_refuses_bad_shapes_before_any_upload():
    from poseprobe_amd import evaluation as E
    a = np.zeros((12, 12, 3), np.float32)
    with pytest.raises(ValueError, match='shape'):
        E.rgb_ssim(a, np.zeros((12, 13, 3), np.float32), 1.)
    with pytest.raises(ValueError, match='shape'):
        E.rgb_ssim(torch.zeros(2, 12, 12, 3), torch.zeros(12, 12, 3), 1.)
    with pytest.raises(ValueError, match='smaller than the filter'):
        E.rgb_ssim(np.zeros((10, 12, 3), np.float32), np.zeros((10, 12, 3), np.float32), 1.)
    with pytest.raises(ValueError):
        E.rgb_ssim(np.zeros((12, 12), np.float32), np.zeros((12, 12), np.float32), 1.)


def test_pp_ssim_refuses_bad_arguments_before_any_gpu_call():
    from poseprobe_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)                 # never dereferenced: every call below is refused by the host checks
    d = ctypes.c_double

    def call(img0=p, img1=p, V=1, H=16, W=16, C=3, fs=11, sigma=1.5, max_val=1., work=p, work_bytes=1 << 20, out=p, smap=None):
        return L.pp_ssim(img0, img1, V, H, W, C, fs, d(sigma), d(max_val), d(0.01), d(0.03), work, work_bytes, out, smap, None)

    for kw, text in ((dict(img0=None), b'null'), (dict(img1=None), b'null'), (dict(work=None), b'null'), (dict(out=None), b'null'),
                     (dict(H=10), b'smaller than the filter'), (dict(W=10), b'smaller than the filter'), (dict(C=5), b'channels'),
                     (dict(C=0), b'channels'), (dict(fs=34), b'filter_size'), (dict(fs=0), b'filter_size'), (dict(V=0), b'view'),
                     (dict(sigma=0.), b'filter_sigma'), (dict(sigma=float('nan')), b'filter_sigma'),
                     (dict(max_val=float('inf')), b'max_val'), (dict(max_val=-1.), b'max_val'),
                     (dict(work_bytes=7), b'too small'), (dict(work=ctypes.c_void_p(4100)), b'aligned')):
        assert call(**kw) == -1, kw
        assert b'pp_ssim' in L.pp_last_error() and text in L.pp_last_error(), (kw, L.pp_last_error())
    assert call(V=1 << 20, H=1 << 15, W=1 << 15) == -3 and b'tiles' in L.pp_last_error()
    b = ctypes.c_int64()
    assert L.pp_ssim_workspace(3, 16 + 10, 2 * 16 + 10 + 1, 11, ctypes.byref(b)) == 0 and b.value == 8 * 3 * 1 * 3
    assert L.pp_ssim_workspace(1, 10, 16, 11, ctypes.byref(b)) == -1 and L.pp_ssim_workspace(1, 16, 16, 11, None) == -1


def test_ssim_wrapper_refuses_cpu_tensors():
    from poseprobe_amd import ops
    a = torch.zeros(1, 12, 12, 3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.ssim(a, a, 1., 11, 1.5, 0.01, 0.03, torch.zeros(8, dtype=torch.uint8), torch.zeros(1))
