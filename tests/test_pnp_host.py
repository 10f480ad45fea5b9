"""PnP-RANSAC pose initialisation, the part that needs no GPU: the numpy restatement of its semantics against mathematics
(tests/pnp_reference.py - the reference the GPU tests compare with), the sample drawer, and the argument validation of the two
pp_pnp_* entry points (every refusal comes before a launch)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import pnp_reference as R

# (P, outlier fraction, pixel noise sigma, H)
CASES = [(16, 0.0, 0.0, 32), (37, 0.3, 0.5, 64), (64, 0.3, 0.5, 64), (257, 0.4, 1.0, 128), (1000, 0.5, 1.0, 256)]


@functools.lru_cache(maxsize=None)
def case(P, outliers, sigma, H):
    d = R.synthetic(P, outliers, sigma, seed=P)
    samples = R.draw(d['valid'], H, seed=P + 1)
    return d, samples, R.ransac(d['world'], d['pix'], d['valid'], d['intr'], samples)


# ---- 1. the numpy restatement against mathematics ------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,H', [(6, 1), (16, 32), (64, 64)])
def test_reference_recovers_the_generating_pose_without_noise(P, H):
    """float64 inputs as generated (fp32 rounding of the pixels alone, 2^-16 px at 200 px, moves the pose by about 1e-7): every
    hypothesis and the refined result equal the generating pose to 1e-8, every valid row is an inlier."""
    d = R.synthetic(P, seed=P, invalid=0.0 if P == 6 else 0.1, round32=False)
    samples = R.draw(d['valid'], H, seed=P + 1)
    r = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], samples, exact=True)
    assert r['flags'].all() and (r['counts'] == int(d['valid'].sum())).all()
    err_h = float(np.abs(r['poses'] - d['T']).max())
    err = float(np.abs(r['pose64'] - d['T']).max())
    print(f'P={P}: hypotheses within {err_h:.2e}, refined pose within {err:.2e}')
    assert err_h <= 1e-8 and err <= 1e-8
    assert r['info'].tolist() == [int(d['valid'].sum()), 0] and np.array_equal(r['inliers'], d['valid'])


def test_reference_p3p_solutions_reproject_their_three_points():
    d = R.synthetic(257, seed=3, invalid=0.0, round32=False)
    world, pix = d['world'].astype(np.float64), d['pix']
    rng = np.random.RandomState(0)
    worst, n_sol, n_true = 0.0, 0, 0
    for _ in range(300):
        s = rng.choice(len(world), 3, replace=False)
        sols = R.p3p(world[s], R.bearings(pix[s], d['intr']))
        assert 1 <= len(sols) <= 4
        for T in sols:
            depth, e2 = R.project(T, d['intr'], world[s], pix[s])
            assert (depth > 0).all()
            assert abs(np.linalg.det(T[:, :3]) - 1.0) < 1e-9 and np.abs(T[:, :3] @ T[:, :3].T - np.eye(3)).max() < 1e-9
            worst = max(worst, float(np.sqrt(e2.max())))
        n_sol += len(sols)
        n_true += any(np.abs(T - d['T']).max() < 1e-7 for T in sols)       # the generating pose is one of them
    print(f'{n_sol} solutions of 300 triples, worst reprojection {worst:.2e} px')
    assert worst <= 1e-8 and n_true == 300 and n_sol > 300


def test_reference_degenerate_triples_have_no_solution():
    j = R.bearings(np.array([[10.0, 20.0], [200.0, 210.0], [390.0, 100.0]]), R.INTR)
    line = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [3.0, 6.0, 9.0]])
    assert R.p3p(line, j) == []
    assert R.p3p(np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [0.0, 1.0, 0.0]]), j) == []


@pytest.mark.parametrize('P,outliers,sigma,H', CASES)
def test_reference_agrees_with_its_permuted_twin(P, outliers, sigma, H):
    """The same hypotheses solved on the two cyclic permutations of the three points - another quartic, the same solution set:
    no validity flip, no inlier-mask difference, hypothesis poses within 5e-7 (measured: 2e-12 - the Newton polish of the three
    distances removes what the two eliminations lose), refined poses within 1e-12; and nothing sits within 1e-4 px of the
    threshold (the guard of the GPU parity cases)."""
    d, samples, a = case(P, outliers, sigma, H)
    assert a['margin'] > 1e-4
    for shift in (1, 2):
        b = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], samples, shift=shift)
        both = a['flags'] & b['flags']
        dp = float(np.abs(a['poses'][both] - b['poses'][both]).max())
        print(f'P={P} shift={shift}: {int(a["flags"].sum())} valid, hypothesis poses within {dp:.2e}')
        assert np.array_equal(a['flags'], b['flags']) and np.array_equal(a['counts'], b['counts'])
        assert np.array_equal(a['masks'], b['masks']) and np.array_equal(a['info'], b['info'])
        assert dp <= 5e-7
        assert np.abs(a['pose64'] - b['pose64']).max() <= 1e-12


@pytest.mark.parametrize('P,outliers,sigma,H', CASES[1:])
def test_reference_ransac_with_outliers(P, outliers, sigma, H):
    """The winner collects every true inlier (noise of sigma <= 1 px against a threshold of 8 px), ties go to the lowest index,
    ten Gauss-Newton steps are converged, and the result is noise-limited."""
    d, samples, r = case(P, outliers, sigma, H)
    truth = d['valid'].astype(bool) & ~d['outlier']
    assert (r['inliers'].astype(bool) | ~truth).all()
    assert not r['inliers'][d['valid'] == 0].any()
    count, best = r['info']
    assert count == r['counts'].max() == r['inliers'].sum() and best == int(np.flatnonzero(r['counts'] == count)[0])
    r20 = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], samples, refine_iters=20)
    assert np.abs(r20['pose64'] - r['pose64']).max() <= 1e-14
    angle, dist = R.pose_distance(r['pose64'], d['T'])
    print(f'P={P}: {count} inliers, {int((r["counts"] == count).sum())} hypotheses tie, {angle:.3f} deg, |dt| = {dist:.2e}')
    if P == 64:
        assert angle <= 0.2 and dist <= 4e-3


def test_reference_failure_returns_the_fallback():
    d, samples, _ = case(37, 0.3, 0.5, 64)
    fb = np.arange(12, dtype=np.float32).reshape(3, 4)
    r = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], samples, min_inliers=30, fallback=fb)
    assert np.array_equal(r['w2c'], fb) and not r['inliers'].any() and r['info'].tolist() == [0, -1]
    r = R.ransac(d['world'], d['pix'], np.zeros(37, np.uint8), d['intr'], samples)
    assert (r['counts'] == -1).all() and r['info'].tolist() == [0, -1] and np.array_equal(r['w2c'], np.eye(4, dtype=np.float32)[:3])


# ---- 2. the sample drawer --------------------------------------------------------------------------------------------------------
def test_draw_samples_rows_are_distinct_valid_and_reproducible():
    from poseprobe_amd import pnp
    valid = torch.tensor(R.synthetic(257, seed=1, invalid=0.4)['valid'])
    s = pnp.draw_samples(valid, 300, torch.Generator().manual_seed(5))
    assert s.shape == (300, 4) and s.dtype == torch.int32
    assert bool(valid[s.long()].all())
    assert all(len(set(row)) == 4 for row in s.tolist())
    assert torch.equal(s, pnp.draw_samples(valid, 300, torch.Generator().manual_seed(5)))
    assert not torch.equal(s, pnp.draw_samples(valid, 300, torch.Generator().manual_seed(6)))
    seen = torch.bincount(s.flatten().long(), minlength=257)
    assert bool((seen[valid == 0] == 0).all()) and int((seen > 0).sum()) > 0.9 * int(valid.sum())    # every valid row can be drawn


def test_draw_samples_small_budget_and_exactly_four_valid_rows(monkeypatch):
    from poseprobe_amd import pnp
    valid = torch.zeros(40, dtype=torch.uint8)
    valid[[3, 8, 21, 34]] = 1
    monkeypatch.setattr(pnp, '_KEY_BUDGET', 40 * 7)                       # several chunks of hypotheses
    s = pnp.draw_samples(valid, 23, torch.Generator().manual_seed(0))
    assert s.shape == (23, 4) and all(sorted(row) == [3, 8, 21, 34] for row in s.tolist())


def test_draw_samples_with_three_valid_rows_yields_invalid_hypotheses():
    """Fewer than four valid rows: nothing raises and nothing is read on the host; each hypothesis holds the three valid rows and
    one invalid row, which the kernel (and the reference) mark invalid."""
    from poseprobe_amd import pnp
    d = R.synthetic(16, seed=2)
    valid = np.zeros(16, np.uint8)
    valid[[2, 5, 11]] = 1
    s = pnp.draw_samples(torch.tensor(valid), 9, torch.Generator().manual_seed(0)).numpy()
    assert s.shape == (9, 4) and all(len(set(row)) == 4 and set(row[:3]) == {2, 5, 11} for row in s.tolist())
    r = R.ransac(d['world'], d['pix'], valid, d['intr'], s)
    assert not r['flags'].any() and r['info'].tolist() == [0, -1]
    with pytest.raises(ValueError, match='at least 4'):
        pnp.draw_samples(torch.ones(3), 9)


# ---- 3. argument validation (before any GPU call) --------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(4096)         # never dereferenced: every call below is refused first
P_MAX, H_MAX = 1 << 22, 1 << 16


def _refused(rc, name, code=-1):
    from poseprobe_amd import _lib
    assert rc == code, (name, rc)
    assert name.encode() in _lib.lib().pp_last_error()


def test_pnp_workspace_values_and_refusals():
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    b = ctypes.c_int64(-1)
    _refused(L.pp_pnp_workspace(16, 8, None), 'pp_pnp_workspace')
    for P, H in ((3, 8), (0, 8), (-1, 8), (16, 0), (16, -5)):
        _refused(L.pp_pnp_workspace(P, H, ctypes.byref(b)), 'pp_pnp_workspace')
    _refused(L.pp_pnp_workspace(P_MAX + 1, 8, ctypes.byref(b)), 'pp_pnp_workspace', -3)
    _refused(L.pp_pnp_workspace(16, H_MAX + 1, ctypes.byref(b)), 'pp_pnp_workspace', -3)
    assert b.value == -1
    r = lambda n: (n + 255) // 256 * 256
    for P, H in ((4, 1), (16, 32), (2049, 320), (P_MAX, H_MAX)):
        assert ops.pnp_workspace(P, H) == r(96 * H) + 2 * r(4 * H)         # 12 doubles, a flag and a count per hypothesis
    with pytest.raises(_lib.PoseProbeError, match='at least 4 rows'):
        ops.pnp_workspace(3, 8)


def test_pnp_ransac_validates_before_any_gpu_call():
    from poseprobe_amd import _lib, ops
    L = _lib.lib()
    P, H = 16, 8
    need = ops.pnp_workspace(P, H)
    names = ('world', 'pix', 'valid', 'intr', 'samples', 'fallback', 'work', 'w2c', 'inliers', 'info')

    def call(P=P, H=H, thr=8.0, refine=10, min_inliers=6, work_bytes=need, **ptr):
        a = {n: FAKE for n in names}
        a.update(ptr)
        return L.pp_pnp_ransac(a['world'], a['pix'], a['valid'], P, a['intr'], a['samples'], H, thr, refine, min_inliers,
                               a['fallback'], a['work'], work_bytes, a['w2c'], a['inliers'], a['info'], None)

    for n in names:
        if n != 'valid':                                                  # (a null `valid` means: every row is valid)
            _refused(call(**{n: None}), 'pp_pnp_ransac')
            assert b'null' in L.pp_last_error()
    for P_bad in (3, 0, -7):
        _refused(call(P=P_bad), 'pp_pnp_ransac')
    for H_bad in (0, -1):
        _refused(call(H=H_bad), 'pp_pnp_ransac')
    _refused(call(P=P_MAX + 1), 'pp_pnp_ransac', -3)
    _refused(call(H=H_MAX + 1, work_bytes=1 << 40), 'pp_pnp_ransac', -3)
    _refused(call(work_bytes=need - 1), 'pp_pnp_ransac')
    assert b'workspace' in L.pp_last_error()
    _refused(call(work=ctypes.c_void_p(4100)), 'pp_pnp_ransac')          # not 16-byte aligned
    for kw in (dict(thr=0.0), dict(thr=-1.0), dict(thr=float('nan')), dict(thr=float('inf')), dict(refine=-1), dict(refine=1001),
               dict(min_inliers=0)):
        _refused(call(**kw), 'pp_pnp_ransac')


def test_wrappers_refuse_cpu_tensors():
    from poseprobe_amd import ops, pnp
    d = R.synthetic(16, seed=0)
    world, pix, intr = torch.tensor(d['world']), torch.tensor(d['pix']), torch.tensor(d['intr'])
    with pytest.raises(RuntimeError, match='CUDA'):
        pnp.solve_pnp_ransac(world, pix, intr)
    work = torch.empty(ops.pnp_workspace(16, 4), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.pnp_ransac(world, pix, None, intr, torch.zeros(4, 4, dtype=torch.int32), 8.0, 10, 6, torch.eye(4)[:3].contiguous(), work,
                       torch.empty(3, 4), torch.empty(16, dtype=torch.uint8), torch.empty(2, dtype=torch.int32))
    poses, flags, counts = ops.pnp_workspace_views(work, 4)
    assert poses.shape == (4, 3, 4) and poses.dtype == torch.float64 and flags.shape == counts.shape == (4,)
    assert flags.data_ptr() - work.data_ptr() == 512 and counts.data_ptr() - work.data_ptr() == 768


def test_trainer_docstring_names_the_initialiser():
    from poseprobe_amd import pnp, trainer
    assert 'pnp.PnPInitialiser' in trainer.DualBranchTrainer.__init__.__doc__
    assert callable(pnp.PnPInitialiser)
