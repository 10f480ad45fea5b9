"""Seeded inputs of tests/test_hip_scene_ray_kernels.py (numpy float32 only, no GPU): compositing rays, coarse weights of the fine
sampler, encoding rays and pose-fold batches, with the edge cases planted at known places.  tests/test_scene_ray_reference.py
checks on the CPU that the planted cases have the properties the GPU tests rest on."""
import numpy as np

F32 = np.float32

# ------------------------------------------------------------------------------------------------------------------ compositing
COMPOSITE_S = (1, 2, 63, 64, 65, 128, 200, 512)          # one chunk, its edges, two, four (ragged) and the limit of eight
COMPOSITE_R = 13                                          # four rays per work-group: the last group holds one
NEAR, FAR = 0.4, 2.4


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def tie_start(S):
    """First of the three equal depths of ray 6: across the 64-sample boundary where the ray has one."""
    return 62 if S >= 65 else S // 2


def composite_case(S, R=COMPOSITE_R, seed=0):
    """-> dict of float32 arrays: rgb_s [R,S,3], density [R,S], depth [R,S], ray [R,3], the upstream gradients g_rgb [R,3],
    g_depth, g_opacity [R], g_weights [R,S] (random, none of them zero).  Every ray starts generic (depths jittered-stratified in
    [0.4, 2.4], density softplus(2 randn), colours in [0, 1], |ray| in [0.7, 1.7]); ray k < 10 (as far as R reaches) is then
      1 density 0 on all but the last sample     2 density 1e4 at sample min(3, S - 1)     3 density 0 everywhere
      4 ray x 1e-3     5 ray x 1e3     6 three equal consecutive depths (S > 4)     7 density 1e-12 everywhere
      8 density x 40     9 the last sample's density exactly 0
    and rays 0, 10, 11, ... stay generic."""
    rng = np.random.RandomState(1000 * seed + 7 * S + R)
    depth = (rng.rand(R, S) + np.arange(S)) / S * (FAR - NEAR) + NEAR
    density = np.logaddexp(0.0, 2.0 * rng.normal(size=(R, S)))
    rgb_s = rng.rand(R, S, 3)
    ray = _unit(rng, R) * rng.uniform(0.7, 1.7, (R, 1))
    if R > 1:
        density[1, :-1] = 0.0
    if R > 2:
        density[2, min(3, S - 1)] = 1e4
    if R > 3:
        density[3] = 0.0
    if R > 4:
        ray[4] *= 1e-3
    if R > 5:
        ray[5] *= 1e3
    if R > 6 and S > 4:
        k = tie_start(S)
        depth[6, k + 1:k + 3] = depth[6, k]
    if R > 7:
        density[7] = 1e-12
    if R > 8:
        density[8] *= 40.0
    if R > 9:
        density[9, -1] = 0.0
    out = dict(rgb_s=rgb_s, density=density, depth=depth, ray=ray)

    def nz(*shape):                                        # random, |g| >= 0.1: no upstream gradient is zero
        g = rng.normal(size=shape)
        return g + np.sign(g) * 0.1

    out.update(g_rgb=nz(R, 3), g_depth=nz(R), g_opacity=nz(R), g_weights=nz(R, S))
    out = {k: np.ascontiguousarray(v, dtype=F32) for k, v in out.items()}
    assert all((out[k] != 0).all() for k in ('g_rgb', 'g_depth', 'g_opacity', 'g_weights'))
    return out


# ----------------------------------------------------------------------------------------------------------------- fine sampler
PDF_N = (1, 2, 63, 64, 65, 200, 256)
PDF_NF = (1, 64, 65, 256)
PDF_R = 10
PDF_RANGE = (float(F32(0.45)), float(F32(2.7)))           # the float32 values the kernel receives; neither is a dyadic fraction
PDF_GRIDS = [(per_ray, det) for per_ray in (False, True) for det in (True, False)]
SMOOTH_RAYS = (0, 5)


def pdf_weights(N, seed=0):
    """Coarse weights [PDF_R, N]: 0 generic (0.02 rand)   1 one-hot, 0.9 in bin N // 2   2 all zero   3 80 % of the bins zeroed
    4 every bin 1e-7 of one dominant bin   5 uniform 1 / N   6 total mass about the 1e-6 of the denominator   7 leading half zero
    8 trailing half zero   9 generic."""
    rng = np.random.RandomState(50 + 1000 * seed + N)
    w = 0.02 * rng.rand(PDF_R, N)
    w[1] = 0.0
    w[1, N // 2] = 0.9
    w[2] = 0.0
    dead = rng.permutation(N)[:int(0.8 * N)]
    w[3, dead] = 0.0
    w[4] = 0.5e-7
    w[4, (2 * N) // 3] = 0.5
    w[5] = 1.0 / N
    w[6] = rng.rand(N) * 2e-6 / N
    w[7, :N // 2] = 0.0
    w[8, N - N // 2:] = 0.0
    return np.ascontiguousarray(w, dtype=F32)


def pdf_grid(Nf, per_ray, det, seed=0):
    """[Nf + 1] or [PDF_R, Nf + 1]: linspace(0, 1), or uniform draws x 0.999 in no order (no u reaches 1) whose first two entries are
    0: u_0 = 0 lies ON the cdf's leading plateau (cdf[0] = 0, and every further zero bin), the tie that tells searchsorted's
    right = True from left - on the all-zero ray the sample belongs on dmax, not on dmin."""
    rng = np.random.RandomState(90 + 1000 * seed + 2 * Nf + per_ray)
    if det:
        g = np.linspace(0, 1, Nf + 1, dtype=F32)
        return np.ascontiguousarray(np.broadcast_to(g, (PDF_R, Nf + 1))) if per_ray else g
    g = (rng.rand(*((PDF_R, Nf + 1) if per_ray else (Nf + 1,))) * 0.999).astype(F32)
    g[..., :2] = 0.0
    return g


def n_below(N):
    return N // 2


def pdf_depths(N, inside, seed=0):
    """Coarse depths [PDF_R, N] in no order.  inside: jittered-stratified in the range, as in training, with two equal depths
    (N >= 2) and one equal to dmax (N >= 3).  Otherwise all outside the range: n_below(N) strictly below dmin (two of them equal,
    N >= 4), the others at or above dmax, one of them dmax itself."""
    lo, hi = PDF_RANGE
    rng = np.random.RandomState(70 + 1000 * seed + 2 * N + inside)
    if inside:
        d = ((rng.rand(PDF_R, N) + np.arange(N)) / N * (hi - lo) + lo).astype(F32)
        d = np.clip(d, F32(lo), F32(hi))
        if N >= 2:
            d[:, 1] = d[:, 0]
        if N >= 3:
            d[:, N - 1] = F32(hi)
    else:
        nb = n_below(N)
        below = (lo - 0.05 - rng.rand(PDF_R, nb)).astype(F32)
        above = (hi + 0.05 + rng.rand(PDF_R, N - nb)).astype(F32)
        if nb >= 2:
            below[:, 1] = below[:, 0]
        above[:, 0] = F32(hi)
        d = np.concatenate([below, above], 1)
    for r in range(PDF_R):
        d[r] = d[r, rng.permutation(N)]
    return np.ascontiguousarray(d, dtype=F32)


# --------------------------------------------------------------------------------------------------------------------- encoding
ENCODE_SHAPES = ((5, 3), (3, 7), (1, 2), (2, 66))         # M = R * S: 15, 21 (no multiple of 4), 2, 132 (more than one work-group)
ENCODE_PROGRESS = (0.45, 0.565, 1.0)                      # with the window (0.4, 0.7): partly open, half open, fully open
BARF_C2F = (0.4, 0.7)


def encode_case(R, S, seed=0):
    """-> center [R,3], ray [R,3], depth [R,S].  Ray 0 lies along an axis; ray 1 (ray 0 where R = 1) has length 1e-3."""
    rng = np.random.RandomState(30 + 1000 * seed + 10 * R + S)
    center = rng.normal(size=(R, 3)) * 0.3
    ray = _unit(rng, R) * rng.uniform(0.7, 1.7, (R, 1))
    ray[0] = (0.0, 0.0, 1.3)
    if R > 1:
        ray[1] *= 1e-3 / np.linalg.norm(ray[1])
    else:
        ray[0] = (0.0, 1e-3, 0.0)
    depth = (rng.rand(R, S) + np.arange(S)) / S * (FAR - NEAR) + NEAR
    return tuple(np.ascontiguousarray(a, dtype=F32) for a in (center, ray, depth))


# -------------------------------------------------------------------------------------------------------------------- pose fold
FOLD_N = (1, 255, 256, 257, 1000)                         # around the 256 threads of the work-group, and a ragged fourth pass
FOLD_V = (1, 3)
FOLD_ROWS = 5


def fold_case(V, N, seed=0):
    """-> g_ray, g_center, dir_cam [V, N, 3]"""
    rng = np.random.RandomState(10 + 1000 * seed + 10 * N + V)
    return tuple(rng.normal(size=(V, N, 3)).astype(F32) for _ in range(3))
