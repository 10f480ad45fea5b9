"""Seeded inputs of tests/test_hip_ray_kernels.py (numpy only, no GPU): poses, sampler rays and loss batches with the edge
cases planted at known places.  tests/test_ray_reference.py checks, with the oracle alone, that the sampler inputs have the
properties their tests rest on."""
import numpy as np

from poseprobe_amd import synthetic as syn
from tests.ray_reference import BCE_HI, BCE_LO, ENT_HI, ENT_LO

F32 = np.float32
THETAS = (0.0, 1e-4, 1e-2, 1.0, 3.0)                   # rotation magnitudes, cycled over the views


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _rigid(rng, n):
    """n random rigid poses [n,3,4]: rotation by a random angle about a random axis (Rodrigues, float64), O(1) translation."""
    ax, th = _unit(rng, n), rng.uniform(0.2, 3.0, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 2] = -ax[:, 2], ax[:, 1], -ax[:, 0]
    K = K - K.transpose(0, 2, 1)
    R = np.eye(3) + np.sin(th)[:, None, None] * K + (1 - np.cos(th))[:, None, None] * (K @ K)
    return np.concatenate([R, rng.uniform(-2, 2, (n, 3, 1))], -1)


def pose_case(V, masked, seed=0):
    """-> se3 [V,6], w2c_init [V,3,4] (float32), refine_mask [V] int32 or None.  |w| of view v is THETAS[v % 5] (view 0: w = 0
    exactly), translations are O(1); the mixed mask fixes view 0 and about a third of the others."""
    rng = np.random.RandomState(100 + seed + V)
    th = np.array([THETAS[v % len(THETAS)] for v in range(V)])
    se3 = np.concatenate([_unit(rng, V) * th[:, None], rng.uniform(-1, 1, (V, 3))], 1).astype(F32)
    long = np.linalg.norm(se3[:, :3].astype(np.float64), axis=1) > th              # float32 rounding must not push |w| past 3
    se3[long, :3] *= F32(1 - 1e-6)
    init = _rigid(rng, V).astype(F32)
    mask = None
    if masked:
        mask = (rng.rand(V) < 0.65).astype(np.int32)
        mask[0] = 0
        if V > 1:
            mask[1] = 1
    return se3, init, mask


# --------------------------------------------------------------------------------------------------------------------- samplers
SAMPLER_SIZES = [1, 4, 5, 1023, 1024, 1025, 2100]
# (grid size G of helpers.scene_for(G, stepsize=0.5), rays, kind): G = 24 has 87 sample slots per ray (two 64-lane chunks), G = 40 has
# 143 (three); 1023 / 1024 / 1025 / 2100 rays cross the 1024-entry pass of the count scan; one batch in which every ray misses
SAMPLER_CASES = [(24, n, 'mixed') for n in SAMPLER_SIZES] + [(24, 1025, 'miss'), (40, 5, 'mixed')]
N_SPECIAL = 8
CENTRE = ((syn.XYZ_MIN.astype(np.float64) + syn.XYZ_MAX) / 2)


def _special_rays():
    """Eight rays in float64, (origin, direction, jitter or None):
    0 along the box diagonal (the longest run of kept samples), 1 one zero direction component, 2 two zero components, 3 aimed
    past the box, 4 origin inside the box, 5 pointing away from the box, 6 an ordinary ray with jitter 0, 7 one with the largest
    float32 below 1."""
    c, diag = CENTRE, (syn.XYZ_MAX - syn.XYZ_MIN).astype(np.float64)
    diag = diag / np.linalg.norm(diag)
    d1 = np.array([0.0, 0.6, 0.8])
    d2 = np.array([0.0, 0.0, 1.0])
    d3 = np.array([0.36, 0.48, 0.8])
    aim = np.array([0.31, -0.22, 0.17])
    d6 = (c + aim - (c - 2.0 * d3)) / np.linalg.norm(c + aim - (c - 2.0 * d3))
    return [(c - 2.0 * diag, diag, None),
            (c + [0.21, 0.0, 0.0] - 2.0 * d1, d1, None),
            (c + [-0.17, 0.33, 0.0] - 2.0 * d2, d2, None),
            (c - 2.0 * d3, np.array([0.8, 0.36, 0.48]), None),
            (c + [0.1, -0.2, 0.15], np.array([0.48, 0.8, -0.36]), None),
            (c - 2.0 * d3, -d3, None),
            (c - 2.0 * d3, d6, 0.0),
            (c - 1.8 * d1 + [0.05, 0.1, 0.0], np.array([0.1, 0.55, 0.83]) / np.linalg.norm([0.1, 0.55, 0.83]),
             float(np.nextafter(F32(1), F32(0))))]


def sampler_rays(n_rays, kind='mixed', seed=0):
    """-> rays_o, rays_d [n,3], jitter [n] (float32).  'mixed': unit rays from radius 1.5 - 2.5 aimed at uniform points of the
    box, with the special rays (above) planted at the front - as many as fit; from 1023 rays on also at the very end, behind the
    scan's first pass of 1024.  'miss': every ray starts at radius 2 and points away from the box."""
    rng = np.random.RandomState(200 + seed + n_rays)
    o = CENTRE + _unit(rng, n_rays) * rng.uniform(1.5, 2.5, (n_rays, 1))
    jit = rng.rand(n_rays)
    if kind == 'miss':
        d = (o - CENTRE) + 0.3 * _unit(rng, n_rays)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return o.astype(F32), d.astype(F32), jit.astype(F32)
    assert kind == 'mixed'
    p = rng.uniform(syn.XYZ_MIN, syn.XYZ_MAX, (n_rays, 3))
    d = (p - o) / np.linalg.norm(p - o, axis=1, keepdims=True)
    sp = _special_rays()
    places = list(range(min(N_SPECIAL, n_rays)))
    if n_rays >= 1023:
        places += list(range(n_rays - N_SPECIAL, n_rays))
    for at in places:
        so, sd, sj = sp[at % N_SPECIAL]
        o[at], d[at] = so, sd
        if sj is not None:
            jit[at] = sj
    return o.astype(F32), d.astype(F32), jit.astype(F32)


# ----------------------------------------------------------------------------------------------------------------------- losses
ALAST_SEEDS = (0.0, 1e-7, ENT_LO, 0.5, ENT_HI, 1.0)        # below / at / inside / at / above the entropy clamp
CW_SEEDS = (0.0, BCE_LO, 0.5, BCE_HI, 1.0)


def ray_loss_case(n_rays, seed=0):
    """-> dict(rgbm [n,3], alast [n], cw [n], target [n,3], mask [n]) float32.  The clamp seeds are written round-robin from the
    end of the batch backwards (so a batch of one ray holds the last seed of each list); masks are random 0/1 with ray 0 set."""
    rng = np.random.RandomState(300 + seed + n_rays)
    d = dict(rgbm=rng.rand(n_rays, 3), alast=rng.uniform(0.01, 0.99, n_rays), cw=rng.uniform(0.01, 0.99, n_rays),
             target=rng.rand(n_rays, 3), mask=(rng.rand(n_rays) < 0.6).astype(np.float64))
    d['mask'][0] = 1.0
    for key, seeds in (('alast', ALAST_SEEDS), ('cw', CW_SEEDS)):
        for k in range(min(n_rays, 2 * len(seeds))):          # every seed twice where they fit: once per mask value, mostly
            d[key][n_rays - 1 - k] = seeds[(len(seeds) - 1 - k) % len(seeds)]
    if n_rays >= 2 * len(ALAST_SEEDS):
        d['mask'][n_rays - 2 * len(ALAST_SEEDS):] = np.arange(2 * len(ALAST_SEEDS)) % 2
    return {k: v.astype(F32) for k, v in d.items()}


def sample_loss_case(capacity, seed=0):
    """-> dict(gradient [c,3], grad_deform [c,9], warp_out [c,16], sdf_deform [c]) float32 with, where the rows exist: row 0 a zero
    gradient, row 1 the gradient (1, 0, 0), row 2 a zero middle row of grad_deform, row 3 a zero correction, row 4 a zero
    sdf_deform; the same five again in the last rows."""
    rng = np.random.RandomState(400 + seed + capacity)
    d = dict(gradient=rng.normal(0, 0.8, (capacity, 3)), grad_deform=rng.normal(0, 0.3, (capacity, 9)),
             warp_out=rng.normal(0, 0.2, (capacity, 16)), sdf_deform=rng.normal(0, 0.1, capacity))
    for base in (0, capacity - 5):
        if base < 0:
            continue
        for k in range(min(5, capacity - base)):
            r = base + k
            if k == 0:
                d['gradient'][r] = 0.0
            elif k == 1:
                d['gradient'][r] = (1.0, 0.0, 0.0)
            elif k == 2:
                d['grad_deform'][r, 3:6] = 0.0
            elif k == 3:
                d['warp_out'][r, 3] = 0.0
            else:
                d['sdf_deform'][r] = 0.0
    return {k: v.astype(F32) for k, v in d.items()}
