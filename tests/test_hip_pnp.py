"""PnP-RANSAC pose initialisation on the GPU (poseprobe_amd.pnp, csrc/pp_pnp.hip) against the numpy restatement of its semantics
(tests/pnp_reference.py, itself checked against mathematics in tests/test_pnp_host.py): parity on the same samples, the edge
cases of the semantics, determinism and memory discipline, and the initialiser end to end - on a model and through the trainer."""
import functools

import numpy as np
import pytest
import torch

from tests import pnp_reference as R
from tests.helpers import load

pytestmark = pytest.mark.gpu

# (P, H): (outlier fraction, pixel noise sigma, invalid fraction).  A single hypothesis; P and H off the wave (64) and work-group
# (256) sizes; rows beyond one pass of a work-group's stride.
CASES = {(6, 1): (0.0, 0.0, 0.0), (16, 32): (0.0, 0.0, 0.1), (37, 64): (0.3, 0.5, 0.1), (64, 65): (0.3, 0.5, 0.1),
         (257, 128): (0.4, 1.0, 0.1), (1000, 256): (0.5, 1.0, 0.1), (2049, 320): (0.5, 1.0, 0.1)}
GUARD = 65536


@functools.lru_cache(maxsize=None)
def case(P, H):
    """(inputs, samples, reference result) - computed once, read-only.  Built with the guard of the parity test: no valid row's
    error within 1e-4 px of the threshold under any hypothesis (another seed otherwise)."""
    outliers, sigma, invalid = CASES[(P, H)]
    d = R.synthetic(P, outliers, sigma, seed=P, invalid=invalid)
    samples = R.draw(d['valid'], H, seed=P + 1)
    ref = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], samples)
    assert ref['margin'] > 1e-4, f'case {(P, H)}: a row sits {ref["margin"]:.1e} px from the threshold - pick another seed'
    for a in list(d.values()) + [samples] + [v for v in ref.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return d, samples, ref


def run(d, samples, reproj_error=8.0, refine_iters=10, min_inliers=6, fallback=None, valid='own'):
    """One call through ops.pnp_ransac with every output and the workspace embedded in 64 KB of sentinel bytes.
    -> dict(w2c, inliers, info, poses, flags, counts as numpy; intact = the sentinels survived)."""
    from poseprobe_amd import ops
    dev = 'cuda'
    P, H = len(d['world']), len(samples)
    r = lambda n: (n + 255) // 256 * 256
    nwork = ops.pnp_workspace(P, H)
    sizes = [48, P, 8, nwork]
    offs, o = [], GUARD
    for n in sizes:
        offs.append(o)
        o += r(n) + GUARD
    buf = torch.full((o,), 0xA5, dtype=torch.uint8, device=dev)
    w2c = buf[offs[0]:offs[0] + 48].view(torch.float32).view(3, 4)
    inliers = buf[offs[1]:offs[1] + P]
    info = buf[offs[2]:offs[2] + 8].view(torch.int32)
    work = buf[offs[3]:offs[3] + nwork]
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    fb = np.eye(4, dtype=np.float32)[:3] if fallback is None else fallback
    v = d['valid'] if isinstance(valid, str) else valid
    ops.pnp_ransac(t(d['world'], torch.float32), t(d['pix'], torch.float32), None if v is None else t(v, torch.uint8),
                   t(d['intr'], torch.float32), t(samples, torch.int32), reproj_error, refine_iters, min_inliers, t(fb, torch.float32),
                   work, w2c, inliers, info)
    torch.cuda.synchronize()
    keep = torch.ones(o, dtype=torch.bool, device=dev)
    for off, n in zip(offs, sizes):
        keep[off:off + n] = False
    poses, flags, counts = ops.pnp_workspace_views(work, H)
    c = lambda x: x.cpu().numpy().copy()
    return dict(w2c=c(w2c), inliers=c(inliers), info=c(info), poses=c(poses), flags=c(flags), counts=c(counts),
                intact=bool((buf[keep] == 0xA5).all()), raw=buf.cpu())


def assert_matches_reference(out, ref, name=''):
    """Winner, mask and info exactly, the 12 pose entries within 1e-6 (five fp32 roundings of the largest entry, |t| <= 4: both
    sides converge to the same least-squares minimum in fp64).  Per-hypothesis validity and counts: at most 2 % of the hypotheses
    (at least one) may differ - near-double roots classified differently by another root finder -, none of them the winner or
    tied with it."""
    H = len(ref['counts'])
    differ = (out['flags'].astype(bool) != ref['flags']) | (out['counts'] != ref['counts'])
    dpose = float(np.abs(out['w2c'].astype(np.float64) - ref['w2c']).max())
    print(f'{name}: {int(differ.sum())} of {H} hypotheses differ, info {out["info"].tolist()} / {ref["info"].tolist()}, '
          f'max |d pose| = {dpose:.2e}, bit-equal pose: {np.array_equal(out["w2c"], ref["w2c"])}')
    assert out['intact'], f'{name}: a sentinel byte was overwritten'
    assert differ.sum() <= max(1, int(0.02 * H))
    top = ref['counts'].max()
    assert not (differ & ((ref['counts'] == top) | (out['counts'] == top))).any()
    assert np.array_equal(out['counts'] == -1, out['flags'] == 0)
    assert np.array_equal(out['info'], ref['info'])
    assert np.array_equal(out['inliers'], ref['inliers'])
    assert dpose <= 1e-6


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P,H', list(CASES))
def test_pnp_ransac_matches_the_reference(P, H):
    d, samples, ref = case(P, H)
    out = run(d, samples)
    assert ref['info'][1] >= 0
    assert_matches_reference(out, ref, f'P={P} H={H}')
    both = out['flags'].astype(bool) & ref['flags']
    assert np.abs(out['poses'][both] - ref['poses'][both]).max() <= 1e-6            # the hypotheses' own poses (fp64 on both sides)


def test_solve_pnp_ransac_wrapper_and_null_valid():
    from poseprobe_amd import pnp
    d, samples, ref = case(257, 128)
    t = lambda a: torch.tensor(a, device='cuda')
    w2c, inliers, info = pnp.solve_pnp_ransac(t(d['world']), t(d['pix']), t(d['intr']), valid=t(d['valid']), samples=t(samples))
    assert w2c.is_cuda and inliers.is_cuda and info.is_cuda and w2c.shape == (3, 4) and inliers.dtype == torch.uint8
    assert np.array_equal(info.cpu().numpy(), ref['info']) and np.array_equal(inliers.cpu().numpy(), ref['inliers'])
    assert np.abs(w2c.cpu().numpy().astype(np.float64) - ref['w2c']).max() <= 1e-6
    # own draws: reproducible from the generator, and a good pose on this easy case
    g = lambda: torch.Generator(device='cuda').manual_seed(3)
    a = pnp.solve_pnp_ransac(t(d['world']), t(d['pix']), t(d['intr']), valid=t(d['valid']), n_hypotheses=64, generator=g())
    b = pnp.solve_pnp_ransac(t(d['world']), t(d['pix']), t(d['intr']), valid=t(d['valid']), n_hypotheses=64, generator=g())
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[2][1]) >= 0
    assert R.pose_distance(a[0].cpu().numpy().astype(np.float64), d['T'])[0] < 0.5
    # valid = None: every row counts
    every = np.ones(257, np.uint8)
    s_all = R.draw(every, 40, seed=9)
    ref_all = R.ransac(d['world'], d['pix'], every, d['intr'], s_all)
    assert ref_all['margin'] > 1e-4
    assert_matches_reference(run(d, s_all, valid=None), ref_all, 'valid=None')


# ---- 2. edge cases -----------------------------------------------------------------------------------------------------------------
def test_bad_samples_score_minus_one_and_never_win():
    d, samples, _ = case(37, 64)
    d = {k: np.array(v) for k, v in d.items()}
    ok = np.flatnonzero(d['valid'])
    dead = int(np.flatnonzero(d['valid'] == 0)[0])
    line = ok[-3:]                                                        # an exactly collinear triple (integer coordinates)
    d['world'][line] = np.array([[0, 0, 0], [1, 2, 3], [3, 6, 9]], np.float32)
    a, b, c, e = (int(v) for v in ok[:4])
    bad = np.array([[a, b, a, c], [a, b, c, c], [a, dead, b, c], [a, b, c, dead], [a, b, 37, c], [-1, a, b, c], [a, b, c, 1 << 30],
                    [int(line[0]), int(line[1]), int(line[2]), a], [a, a, a, a]], np.int32)
    s = np.concatenate([bad, np.array(samples)[16:48], bad]).astype(np.int32)
    ref = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], s)
    assert ref['margin'] > 1e-4 and not ref['flags'][:9].any() and not ref['flags'][-9:].any() and ref['info'][1] >= 9
    out = run(d, s)
    assert (out['counts'][:9] == -1).all() and (out['counts'][-9:] == -1).all() and (out['flags'][:9] == 0).all()
    assert 9 <= out['info'][1] < 41
    assert_matches_reference(out, ref, 'bad samples')


def test_points_in_one_plane_still_solve():
    d = R.synthetic(64, 0.3, 0.5, seed=5, planar=True)
    assert len(np.unique(d['world'][:, 2])) == 1
    s = R.draw(d['valid'], 48, seed=6)
    ref = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], s)
    assert ref['margin'] > 1e-4 and ref['info'][0] >= 20
    out = run(d, s)
    assert_matches_reference(out, ref, 'planar')
    angle, dist = R.pose_distance(out['w2c'].astype(np.float64), d['T'])
    assert angle < 1.0 and dist < 0.05


def test_rows_behind_the_camera_are_never_inliers():
    """Rows mirrored through the camera centre project onto their pixel exactly, with negative depth."""
    d = R.synthetic(64, seed=8, invalid=0.0)
    d = {k: np.array(v) for k, v in d.items()}
    Rm, t = d['T'][:, :3], d['T'][:, 3]
    behind = np.arange(0, 64, 4)
    cam = d['world'][behind].astype(np.float64) @ Rm.T + t
    d['world'][behind] = ((-cam - t) @ Rm).astype(np.float32)
    front = np.ones(64, np.uint8)
    front[behind] = 0
    s = R.draw(front, 32, seed=1)
    ref = R.ransac(d['world'], d['pix'], d['valid'], d['intr'], s)
    depth, e2 = R.project(d['T'], d['intr'], d['world'].astype(np.float64), d['pix'].astype(np.float64))
    assert (depth[behind] < 0).all() and (e2[behind] < 1e-4).all()          # inliers but for their depth
    assert ref['margin'] > 1e-4 and ref['info'][0] == 48
    out = run(d, s)
    assert_matches_reference(out, ref, 'behind')
    assert not out['inliers'][behind].any() and out['inliers'].sum() == 48


ODD = np.array([[1.5, -0.0, 3e-39, -7.25], [0.1, 1e30, -2.0, 5.0], [9.0, 0.3, -1e-20, 0.7]], np.float32)   # (-0 and a denormal too)


@pytest.mark.parametrize('why', ['too_few_inliers', 'all_rows_invalid', 'every_hypothesis_invalid'])
def test_failure_writes_the_fallback_an_empty_mask_and_no_winner(why):
    d, samples, ref = case(37, 64)
    samples = np.array(samples)
    kw = {}
    if why == 'too_few_inliers':
        kw['min_inliers'] = int(ref['info'][0]) + 1
    elif why == 'all_rows_invalid':
        kw['valid'] = np.zeros(37, np.uint8)
    else:
        samples[:, 1] = samples[:, 0]
    out = run(d, samples, fallback=ODD, **kw)
    assert out['intact']
    assert out['w2c'].tobytes() == ODD.tobytes()
    assert not out['inliers'].any() and out['info'].tolist() == [0, -1]
    if why != 'too_few_inliers':
        assert (out['counts'] == -1).all()
    else:                                                                # ... and one inlier less is a success
        ok = run(d, samples, fallback=ODD, min_inliers=int(ref['info'][0]))
        assert np.array_equal(ok['info'], ref['info']) and np.array_equal(ok['inliers'], ref['inliers'])


def test_ties_resolve_to_the_lowest_index():
    d, samples, ref = case(64, 65)
    samples = np.array(samples)
    count, best = (int(v) for v in ref['info'])
    assert (ref['counts'] == count).sum() > 1                             # ties are the rule, not the exception
    later = run(d, np.concatenate([samples, samples[best:best + 1]]))     # the winning sample again at a higher index
    assert later['info'].tolist() == [count, best] and later['counts'][-1] == count
    first = run(d, np.concatenate([samples[best:best + 1], samples]))     # ... and at index 0
    assert first['info'].tolist() == [count, 0]
    assert np.array_equal(first['inliers'], later['inliers']) and first['w2c'].tobytes() == later['w2c'].tobytes()


# ---- 3. determinism and memory -------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bits_and_leave_the_sentinels_alone():
    d, samples, ref = case(2049, 320)
    a, b = run(d, samples), run(d, samples)
    assert a['intact'] and b['intact']
    for k in ('w2c', 'inliers', 'info', 'poses', 'flags', 'counts'):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert torch.equal(a['raw'], b['raw'])                                # the whole buffer, workspace padding included
    assert np.array_equal(a['info'], ref['info'])


# ---- 4. the initialiser on a model and through the trainer -------------------------------------------------------------------------
RK = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, inverse_y=True, flip_x=False, flip_y=False)


def _matches(model, K, w2c_a, w2c_b, lo, hi, n, seed):
    """A pixel grid in view A, its surface points from the model's own query, their projections under the pose of view B with a
    quarter of them replaced by random pixels 30 to 100 px away.  -> (pix_a, pix_b, conf, hit, replaced)"""
    from poseprobe_amd import camera, recon_utils
    dev = 'cuda'
    ax = torch.linspace(lo, hi, n, device=dev) + 0.25                     # sub-pixel positions
    pix_a = torch.stack(torch.meshgrid(ax, ax, indexing='xy'), -1).reshape(-1, 2)
    o, dd = recon_utils.get_ray_dir(pix_a[None], K[None], c2w=camera.pose.invert(w2c_a[None]), inverse_y=True, flip_x=False,
                                    flip_y=False, mode='no_center')
    pts, hit, _ = model.query_sdf_point_wocuda(o.reshape(-1, 3).contiguous(), dd.reshape(-1, 3).contiguous(), global_step=None,
                                               keep_dim=True, **RK)
    cam = pts.double() @ w2c_b[:, :3].double().T + w2c_b[:, 3].double()
    pix_b = torch.stack([K[0, 0] * cam[:, 0] / cam[:, 2] + K[0, 2], K[1, 1] * cam[:, 1] / cam[:, 2] + K[1, 2]], -1)
    pix_b = torch.where(hit[:, None], pix_b, torch.zeros_like(pix_b)).float()
    g = torch.Generator().manual_seed(seed)
    replaced = (torch.arange(len(pix_a)) % 4 == 1).to(dev)
    radius, phi = 30.0 + 70.0 * torch.rand(len(pix_a), generator=g), 6.2831853 * torch.rand(len(pix_a), generator=g)
    off = torch.stack([radius * torch.cos(phi), radius * torch.sin(phi)], -1).to(dev)
    pix_b = torch.where(replaced[:, None], pix_b + off, pix_b)
    return pix_a, pix_b, torch.ones(len(pix_a), device=dev), hit, replaced


def test_initialiser_recovers_the_pose_of_the_joining_view():
    from poseprobe_amd import pnp
    from poseprobe_amd import synthetic as syn
    from tests.test_hip_dropin import make_model
    model = make_model(load('query_g24.npz'))
    cams = syn.cameras(3)
    w2c_a, w2c_b = torch.tensor(cams[0], device='cuda'), torch.tensor(cams[1], device='cuda')
    Ks = torch.tensor(syn.intrinsics(3, 400, 400), device='cuda')
    pix_a, pix_b, conf, hit, replaced = _matches(model, Ks[0], w2c_a, w2c_b, 130.0, 270.0, 16, seed=0)
    n_hit = int((hit & ~replaced).sum())
    print(f'{int(hit.sum())} of {len(hit)} rays hit the surface, {n_hit} of them keep their match')
    assert n_hit >= 32
    init = pnp.PnPInitialiser(model, {1: (pix_a, pix_b, conf), 2: (pix_a[:0], pix_b[:0], conf[:0])}, Ks, RK, n_hypotheses=64, seed=0)
    out = init(1, w2c_a.cpu())
    assert out.is_cuda and out.shape == (3, 4) and out.dtype == torch.float32
    err = float((out - w2c_b).abs().max())
    count, best = init.last['info'].tolist()
    print(f'pose error {err:.2e}, {count} inliers, hypothesis {best}, {int(init.last["n_valid"])} valid rows')
    assert int(init.last['n_valid']) == int(hit.sum()) and best >= 0 and count == n_hit
    assert err <= 1e-4
    # no matches at all: the previous pose, bit for bit
    again = init(2, w2c_a.cpu())
    assert torch.equal(again.cpu(), w2c_a.cpu()) and init.last['info'].tolist() == [0, -1]
    # matches that agree on nothing: the fallback as well, this time written by the kernel
    g = torch.Generator().manual_seed(4)
    init.matches[2] = (pix_a, (400.0 * torch.rand(len(pix_a), 2, generator=g)).cuda(), conf)
    again = init(2, w2c_a.cpu())
    assert torch.equal(again.cpu(), w2c_a.cpu()) and init.last['info'].tolist() == [0, -1]


def test_trainer_hands_the_joining_view_to_the_initialiser():
    from poseprobe_amd import bg_nerf, ops, pnp
    from poseprobe_amd.trainer import DualBranchTrainer
    from tests.test_hip_step import build_engine
    d = load('forward_g24_s10.npz')
    eng, _ = build_engine(d)
    eng.zero_grads()
    Ks = torch.tensor(d['Ks'], device='cuda')
    w2c = torch.tensor(d['w2c_init'], device='cuda')
    ops.pose_fwd(eng.se3, eng.w2c_init, eng.refine_mask, eng.w2c, eng.c2w, eng.jac)
    # view 1 as it stands now; the replaced rows land outside the 32 x 32 images, which is fine
    pix_a, pix_b, conf, hit, replaced = _matches(eng.voxurf_view(), Ks[1], eng.w2c[1].clone(), w2c[2], 10.0, 22.0, 12, seed=1)
    assert int((hit & ~replaced).sum()) >= 32
    init = pnp.PnPInitialiser(eng, {2: (pix_a, pix_b, conf)}, Ks, RK, n_hypotheses=64, seed=0, reproj_error=2.0)
    returned = []

    def recording(view, prev):
        returned.append((view, init(view, prev)))
        return returned[-1][1]

    opt = bg_nerf.default_options(sample_intvs=16)
    opt.nerf.rand_rays = 96
    torch.manual_seed(3)
    tr = DualBranchTrainer(eng, opt, max_iter=20, incremental_step=2, pose_initialiser=recording)
    for step in range(2):
        tr.train_step(step)
    assert tr.n_active == 2 and not returned
    assert tr._admit_views(2) == 3                                        # the step that admits view 2 begins with this
    assert [v for v, _ in returned] == [2]
    count, best = init.last['info'].tolist()
    print(f'view 2: {count} inliers, hypothesis {best}; |w2c - generating pose| = {float((returned[0][1] - w2c[2]).abs().max()):.2e}')
    assert best >= 0 and count >= 32                                      # PnP succeeded: this is not the fallback
    assert torch.equal(eng.w2c_init[2], returned[0][1]) and float(eng.se3[2].abs().max()) == 0.0
    ops.pose_fwd(eng.se3, eng.w2c_init, eng.refine_mask, eng.w2c, eng.c2w, eng.jac)
    assert float((eng.w2c[2] - w2c[2]).abs().max()) < 0.05                 # two train steps moved view 1 and the surface a little
    tr.train_step(2)                                                      # ... and the rest of that step runs on three views
    assert tr.n_active == 3 and len(returned) == 1 and torch.equal(eng.w2c_init[2], returned[0][1])
