"""Shared by tests/test_evaluation_host.py, tests/test_hip_ssim.py and tools/make_eval_golden.py: a float64 numpy restatement of
the reference's SSIM (lib/utils.py:792-838, without scipy), and the generators of the SSIM and pose cases.  The inputs of a case
are a pure function of its name (RandomState streams), so that the fixture stores only what the reference computed."""
import zlib

import numpy as np

GOLDEN_T = 16            # the tile edge tests/golden/eval_metrics.npz was recorded for (the tests compare it with pp_ssim_tile)


# ------------------------------------------------------------------------------------------------------------------- SSIM
def gaussian_filter(filter_size, filter_sigma):
    """lib/utils.py:804-808."""
    hw = filter_size // 2
    shift = (2 * hw - filter_size + 1) / 2
    f_i = ((np.arange(filter_size) - hw + shift) / filter_sigma) ** 2
    filt = np.exp(-0.5 * f_i)
    return filt / np.sum(filt)


def _blur(z, f):
    """Separable `valid` convolution of z [H,W,C] with f along both image axes (columns first, as the reference)."""
    n = len(f)
    rows = sum(f[k] * z[n - 1 - k:z.shape[0] - k] for k in range(n))
    return sum(f[k] * rows[:, n - 1 - k:rows.shape[1] - k] for k in range(n))


def rgb_ssim(img0, img1, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, return_map=False):
    img0, img1 = np.asarray(img0, np.float64), np.asarray(img1, np.float64)
    assert img0.ndim == 3 and img0.shape == img1.shape
    f = gaussian_filter(filter_size, filter_sigma)
    mu0, mu1 = _blur(img0, f), _blur(img1, f)
    mu00, mu11, mu01 = mu0 * mu0, mu1 * mu1, mu0 * mu1
    sigma00 = np.maximum(0., _blur(img0 ** 2, f) - mu00)
    sigma11 = np.maximum(0., _blur(img1 ** 2, f) - mu11)
    sigma01 = _blur(img0 * img1, f) - mu01
    sigma01 = np.sign(sigma01) * np.minimum(np.sqrt(sigma00 * sigma11), np.abs(sigma01))
    c1, c2 = (k1 * max_val) ** 2, (k2 * max_val) ** 2
    ssim_map = ((2 * mu01 + c1) * (2 * sigma01 + c2)) / ((mu00 + mu11 + c1) * (sigma00 + sigma11 + c2))
    return ssim_map if return_map else np.mean(ssim_map)


def _rs(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def _pair(kind, name, H, W, max_val):
    rs = _rs(name)
    x = rs.rand(H, W, 3)
    if kind == 'noise':
        y = np.clip(x + 0.1 * rs.randn(H, W, 3), 0, 1)
    elif kind == 'smooth':                                   # a smooth image against its noisy copy: low variances
        u, v = np.meshgrid(np.linspace(0, 3, W), np.linspace(0, 2, H))
        x = 0.5 + 0.4 * np.stack([np.sin(u + v), np.cos(2 * u), np.sin(v * u)], -1)
        y = np.clip(x + 0.02 * rs.randn(H, W, 3), 0, 1)
    elif kind == 'negated':
        y = 1 - x
    elif kind == 'identical':
        y = x.copy()
    elif kind == 'zeros_ones':
        x, y = np.zeros((H, W, 3)), np.ones((H, W, 3))
    else:
        raise KeyError(kind)
    return x * max_val, y * max_val


def ssim_cases(T):
    """-> list of dict(name, fs, max_val, pairs=[(img0, img1), ...]) (float64 [H,W,3]; more than one pair: a batch).  Shapes are
    functions of the kernel's output tile edge T: one output pixel, 12 x 29, exactly one tile, one pixel more than a tile in
    each axis, and ragged 2 x 3 tiles ((T + 5) x (2 T + 7) outputs) - the last for every kind of input, for the filter sizes
    1, 4 (even) and 33, and for a batch of three different pairs."""
    def ragged(fs):
        return T + 5 + fs - 1, 2 * T + 7 + fs - 1

    spec = [('one_pixel', 'noise', (11, 11), 11, 1.), ('12x29', 'noise', (12, 29), 11, 1.),
            ('one_tile', 'noise', (T + 10, T + 10), 11, 1.), ('tile_plus_one', 'noise', (T + 11, T + 11), 11, 1.),
            ('ragged', 'noise', ragged(11), 11, 1.), ('negated', 'negated', ragged(11), 11, 1.),
            ('identical', 'identical', ragged(11), 11, 1.), ('zeros_ones', 'zeros_ones', ragged(11), 11, 1.),
            ('max255', 'noise', ragged(11), 11, 255.), ('fs1', 'noise', ragged(1), 1, 1.), ('fs4', 'noise', ragged(4), 4, 1.),
            ('fs33', 'noise', ragged(33), 33, 1.)]
    cases = [dict(name=n, fs=fs, max_val=mv, pairs=[_pair(kind, n, H, W, mv)]) for n, kind, (H, W), fs, mv in spec]
    H, W = ragged(11)
    cases.append(dict(name='batch3', fs=11, max_val=1., pairs=[_pair('noise', 'batch3.a', H, W, 1.), _pair('negated', 'batch3.b', H, W, 1.),
                                                                _pair('smooth', 'batch3.c', H, W, 1.)]))
    return cases


# ------------------------------------------------------------------------------------------------------------------ poses
def _rotation(w):
    """Rodrigues: axis-angle [3] -> [3,3]."""
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def invert(pose):
    R = np.swapaxes(pose[..., :3], -1, -2)
    return np.concatenate([R, -R @ pose[..., 3:]], -1)


def ground_truth_poses(B, seed=0):
    """B world-to-camera poses [B,3,4] float64: cameras scattered around the origin at distance 2..3 with random orientation."""
    rs = np.random.RandomState(1000 + 17 * B + seed)
    c2w = []
    for _ in range(B):
        d = rs.randn(3)
        centre = d / np.linalg.norm(d) * rs.uniform(2, 3)
        c2w.append(np.concatenate([_rotation(rs.randn(3)), centre[:, None]], 1))
    return invert(np.array(c2w))


def move_by_sim3(pose_w2c, s, R, t):
    """The poses whose camera-to-world frames are x -> (R^T (x - t)) / s of the given ones: aligning them back to the given ones
    needs exactly the Sim(3) (s, R, t) - centre' s R + t = centre, R R' = R_c2w."""
    c2w = invert(pose_w2c)
    Rm = R.T[None] @ c2w[:, :, :3]
    cm = (R.T[None] @ (c2w[:, :, 3:] - t[None, :, None])) / s
    return invert(np.concatenate([Rm, cm], -1))


def known_sim3(seed=0):
    rs = np.random.RandomState(77 + seed)
    return 1.7, _rotation(np.array([0.4, -0.7, 0.3])), rs.randn(3)


def perturb(pose_w2c, rot_deg, trans, seed, only=None):
    """Right-multiplied camera-to-world noise: rotations of about rot_deg degrees, centre offsets of about `trans`."""
    rs = np.random.RandomState(500 + seed)
    c2w = invert(pose_w2c).copy()
    for i in range(len(c2w)):
        w, d = rs.randn(3) * np.deg2rad(rot_deg) / np.sqrt(3), rs.randn(3) * trans / np.sqrt(3)
        if only is None or i in only:
            c2w[i, :, :3] = c2w[i, :, :3] @ _rotation(w)
            c2w[i, :, 3] += d
    return invert(c2w)


def pose_cases():
    """-> list of dict(name, pose, GT) float64 [B,3,4]: ground truth moved by a known Sim(3) (s = 1.7) and perturbed by about 2
    degrees / 0.05 per pose, for B on both sides of the aligner switch (9 | 10) and of the 10-pose cap of the pair search."""
    out = []
    for B in (3, 9, 10, 25):
        GT = ground_truth_poses(B)
        out.append(dict(name=f'B{B}', pose=perturb(move_by_sim3(GT, *known_sim3()), 2.0, 0.05, B), GT=GT))
    return out
