"""Seeded inputs of tests/test_hip_scene_mlp_kernels.py and tests/test_scene_mlp_reference.py (numpy float32, no GPU): a packed
parameter block, rays, sample depths, band weights and upstream gradients of one pass of the scene branch's MLP chain."""
import math

import numpy as np

from oracle import scene_nerf as SN
from tests.scene_mlp_reference import IN_LD, PADDING, param_offsets

F32 = np.float32
BARF_C2F = (0.4, 0.7)
PROGRESS = {'open': 1.0, 'partly': 0.565, 'closed': 0.4}    # all bands open; 5 of 10 point bands open (one of them halfway);
#                                                             progress at the schedule's start: every point and view band closed
BD = (0.1, 20.0, -30.0)                                     # density bias: raw around 0, on both sides of 20, deep in the negative tail
UPSTREAM = ('random', 'density_only', 'zero')
NEAR, FAR = 0.4, 2.4

# M = R * S around the 64-row tiles of the fused chain, the 128-row GEMM tiles and the 256-row strips of the heads; rays of several
# samples wherever M allows (127 and 257 are prime), S <= 512
SHAPES = ((1, 3), (7, 9), (4, 16), (5, 13), (1, 127), (2, 64), (3, 43), (5, 51), (4, 64), (1, 257), (29, 67))
MEDIUM = (29, 67)
assert [R * S for R, S in SHAPES] == [3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1943]


# (band schedule, bd) of each shape.  raw - bd = a6 . wd falls with |point| (the raw coordinates reach 24 on the longest ray) and
# rises above 0 only on a few per cent of the samples of a ray bundle with open bands: bd = 20 goes to the shapes where both sides
# of 20 are populated (tests/test_scene_mlp_reference.py asserts it), never to a single ray or to closed bands
SETTINGS = (('open', 0.1), ('partly', -30.0), ('closed', 0.1), ('partly', 0.1), ('closed', -30.0), ('open', 0.1), ('closed', -30.0),
            ('open', 20.0), ('partly', 0.1), ('open', -30.0), ('partly', 20.0))
assert len(SETTINGS) == len(SHAPES)
MIN_PER_SIDE = 4                                             # samples with raw > 20, and with raw <= 20, where bd = 20


def second_tile_shape(cus):
    """The smallest R x 127 above 2 cus 64 rows: a fused work-group and a persistent GEMM work-group take a second tile, the last
    tile is ragged."""
    return 2 * cus * 64 // 127 + 1, 127


def second_strip_shape():
    """The smallest R x 128 above 512 x 256 rows: a work-group of the heads' backward kernels takes a second strip."""
    return 512 * 256 // 128 + 1, 128


def band_weights(progress):
    """[14] float32: oracle.scene_nerf.band_weights of the 10 point bands, then of the 4 view bands."""
    return np.concatenate([SN.band_weights(progress, BARF_C2F, L).numpy() for L in (SN.L_3D, SN.L_VIEW)]).astype(F32)


def params(bd, seed=0, padding=0.0):
    """The packed block: Xavier-uniform weights (gain sqrt 2 in front of a ReLU), every bias 0.05 randn as the scene tests randomise
    them, the density bias `bd`, the padding columns `padding`."""
    rng = np.random.RandomState(4000 + seed)
    off = param_offsets()
    flat = np.zeros(off[22], F32)

    def xavier(rows, cols, ld, gain):
        w = np.zeros((rows, ld), F32)
        a = gain * math.sqrt(6.0 / (rows + cols))
        w[:, :cols] = rng.uniform(-a, a, (rows, cols))
        return w

    g = math.sqrt(2.0)
    used = {0: 63, 4: 319}
    for l in range(8):
        w = xavier(256, used.get(l, IN_LD[l]), IN_LD[l], g)
        for c in PADDING.get(f'W{l}', ()):
            w[:, c] = padding
        flat[off[2 * l]:off[2 * l] + w.size] = w.reshape(-1)
        flat[off[2 * l + 1]:off[2 * l + 1] + 256] = 0.05 * rng.normal(size=256)
    flat[off[16]:off[16] + 256] = xavier(1, 256, 256, 1.0)[0]
    flat[off[17]] = bd
    r0 = xavier(128, 283, 288, g)
    r0[:, list(PADDING['R0'])] = padding
    flat[off[18]:off[18] + r0.size] = r0.reshape(-1)
    flat[off[19]:off[19] + 128] = 0.05 * rng.normal(size=128)
    flat[off[20]:off[20] + 384] = xavier(3, 128, 128, 1.0).reshape(-1)
    flat[off[21]:off[21] + 3] = 0.05 * rng.normal(size=3)
    return flat


def case(R, S, progress='open', bd=0.1, upstream='random', seed=0, padding=0.0):
    """-> dict of float32 arrays: flat, center [R,3], ray [R,3] (lengths log-spaced from 1e-3 to 10: ray 0 the shortest, the last
    the longest; one ray: 1e-3), depth [R,S] jittered-stratified in [0.4, 2.4], bands [14], g_rgb [M,3], g_den [M]."""
    rng = np.random.RandomState(1000 * seed + 10 * R + S)
    center = rng.normal(size=(R, 3)) * 0.3
    d = rng.normal(size=(R, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    length = 10.0 ** np.linspace(-3, 1, R) if R > 1 else np.array([1e-3])
    depth = (rng.rand(R, S) + np.arange(S)) / S * (FAR - NEAR) + NEAR
    M = R * S
    g_rgb, g_den = rng.normal(size=(M, 3)), rng.normal(size=M)
    if upstream != 'random':
        g_rgb[:] = 0.0
    if upstream == 'zero':
        g_den[:] = 0.0
    out = dict(center=center, ray=d * length[:, None], depth=depth, g_rgb=g_rgb, g_den=g_den)
    out = {k: np.ascontiguousarray(v, dtype=F32) for k, v in out.items()}
    out.update(flat=params(bd, seed, padding), bands=band_weights(PROGRESS[progress]))
    return out
