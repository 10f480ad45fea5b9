"""Cases, inputs and tolerances shared by tests/test_hip_optim_kernels.py (GPU) and tests/test_optim_reference.py (CPU).

Everything here is CPU-only.  The GPU file runs the kernels on these inputs and compares with tests/optim_reference.py in
float64; the CPU file evaluates the same reference in float32 on the same inputs and checks that every tolerance below is at
least four times that error, which is where the constants come from.

Scalars are rounded to float32 before either side sees them (f32 below): the C ABI carries lr, the betas, eps and the scales as
float, so these are the numbers the kernels receive.  It matters for the betas: the kernels form 1 - beta from the float they
were given (1 - 0.99f = 0.0099999905, 9.5e-7 away from 0.01), and a reference fed the decimal 0.99 would book that input
rounding as a kernel error.
"""
import numpy as np
import torch


def f32(x):
    return float(np.float32(x))


B1, B2, EPS, LR = f32(0.9), f32(0.99), f32(1e-8), f32(0.1)
TV_SCALE = f32(2e-4)          # six neighbour signs * 2e-4 ~ the data gradient's 1e-3: a wrong sign moves every output
CANARY = 777.0

# ---- tolerances ---------------------------------------------------------------------------------------------------------
# Form: assert_close(kernel, float64 reference, rtol=..., atol=0, scaled=...).  p and the first moment are sums of terms of
# either sign, so their budget is relative to the largest entry (`scaled`); the second moment and the TV value are sums of
# non-negative terms, so theirs is relative to the entry itself (`rtol`).
# Each constant = 4 x (largest error of the float32 evaluation of the reference over all cases of that kind), rounded up to one
# significant digit; the measured value stands next to it.  test_optim_reference.py re-measures and asserts 4 x measured <=
# constant.  The older test_grid_tv_adam_step_matches_oracle allows rtol 1e-5 plus atol of ~1e-6..1e-5 of the largest entry on
# p, m and v and rtol 1e-5 on the TV value: all of these are tighter.
TOL = {
    'grid.p': dict(rtol=0.0, scaled=9e-7),       # float32 evaluation 2.04e-7 of the largest entry, x 4 = 8.2e-7
    'grid.m': dict(rtol=0.0, scaled=3e-7),       # 6.99e-8, x 4 = 2.8e-7
    'grid.v': dict(rtol=8e-7, scaled=0.0),       # 1.80e-7 of the entry, x 4 = 7.2e-7
    'grid.tv': dict(rtol=4e-7, scaled=0.0),      # 8.35e-8 (a float32 sum in another order), x 4 = 3.3e-7
    'tv.grad': dict(rtol=0.0, scaled=3e-7),      # 5.75e-8, x 4 = 2.3e-7
    'tv.value': dict(rtol=4e-7, scaled=0.0),     # 8.35e-8, x 4 = 3.3e-7
    'tv.value.serial': dict(rtol=4e-6, scaled=0.0),   # 7.9e-7 (serial_partial_sums below), x 4 = 3.2e-6
    'flat.p': dict(rtol=0.0, scaled=4e-7),       # 9.60e-8 of the segment's largest entry, x 4 = 3.8e-7
    'flat.m': dict(rtol=0.0, scaled=7e-7),       # 1.74e-7, x 4 = 6.9e-7
    'flat.v': dict(rtol=1e-6, scaled=0.0),       # 2.30e-7, x 4 = 9.2e-7
}


def measured(a, ref, kind):
    """Error of `a` against `ref` in the unit of TOL[kind]: max |a - ref| / max |ref| for the `scaled` kinds, max |a - ref| /
    |ref| for the `rtol` kinds (an entry that is exactly 0 in the reference has to be exactly 0)."""
    a = torch.as_tensor(a).detach().cpu().double().reshape(-1)
    ref = torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    err = (a - ref).abs()
    if kind.split('.')[1] in ('v', 'tv', 'value'):
        assert bool((err[ref == 0] == 0).all()), kind
        nz = ref != 0
        return float((err[nz] / ref[nz].abs()).max()) if bool(nz.any()) else 0.0
    return float(err.max() / ref.abs().max())


# ---- grids --------------------------------------------------------------------------------------------------------------
def grid_inputs(shape, seed=0):
    """p, grad, m, v [X,Y,Z,C] float32.  p = 0.1 * randn with exact ties planted by copying values: across EVERY x border
    (hence every chunk border of every chunk count, every slab border and the last plane), and in y and in z on every plane
    (the last one included).  About 5 % of the voxels have grad = m = v = 0 exactly."""
    X, Y, Z, C = shape
    g = torch.Generator().manual_seed(1000 + seed)
    p = torch.randn(X, Y, Z, C, generator=g) * 0.1
    h = max(1, C // 2)
    for x in range(1, X):                           # half of the channels tie with plane x - 1, alternating halves: no chains
        c0 = (x % 2) * (C // 2)
        p[x, x % Y, (3 * x + 1) % Z, c0:c0 + h] = p[x - 1, x % Y, (3 * x + 1) % Z, c0:c0 + h]
    for x in range(X):       # copied FROM the x-tie voxels; where such a write lands on channel 0 or C - 1 of another x tie, that
                             # tie keeps its other channels (test_every_case_has_its_ties_and_zero_voxels counts what is left)
        y, z = x % Y, (3 * x + 1) % Z
        if Y > 1:                                   # channel 0 of a y neighbour ties with it
            p[x, y + 1 if y + 1 < Y else y - 1, z, 0] = p[x, y, z, 0]
        if Z > 1:                                   # the last channel of a z neighbour ties with it
            p[x, y, z + 1 if z + 1 < Z else z - 1, C - 1] = p[x, y, z, C - 1]
    grad = torch.randn(X, Y, Z, C, generator=g) * 1e-3
    m = torch.randn(X, Y, Z, C, generator=g) * 1e-3
    v = torch.rand(X, Y, Z, C, generator=g) * 1e-6
    zero = torch.rand(X, Y, Z, generator=g) < 0.05
    zero.view(-1)[0] = True
    zero.view(-1)[-1] = True
    for t in (grad, m, v):
        t[zero] = 0.0
    return p, grad, m, v


def tie_counts(p):
    """Number of exactly-zero forward differences along x (per border), y and z (per plane)."""
    dx = ((p[1:] - p[:-1]) == 0).flatten(1).sum(1)
    dy = ((p[:, 1:] - p[:, :-1]) == 0).flatten(1).sum(1)
    dz = ((p[:, :, 1:] - p[:, :, :-1]) == 0).flatten(1).sum(1)
    return dx, dy, dz


# (id, shape (X,Y,Z,C), slabs called in turn on one set of buffers, reason)
DENSE_CASES = [
    ('5x6x7x12', (5, 6, 7, 12), [(0, 5)], 'nx < 8: every plane is its own chunk'),
    ('13x5x3x8', (13, 5, 3, 8), [(0, 13)], 'chunk_len 2, 7 chunks, the last chunk has one plane'),
    ('13x5x3x8-slabs', (13, 5, 3, 8), [(0, 1), (1, 6), (6, 13)],
     'one-plane slab, unequal slabs, halo from outside the slab on both sides'),
    ('130x3x5x4', (130, 3, 5, 4), [(0, 130)], '16-chunk branch: chunk_len 9, so 14 chunks of 9 planes and one of 4; q4 = 1'),
    ('130x3x5x4-inner', (130, 3, 5, 4), [(1, 129)], '16-chunk branch at its threshold nx = 128, slab inside the grid'),
    ('16x9x11x12', (16, 9, 11, 12), [(0, 16)], '297 float4 per plane: two tiles, the second partial'),
    ('6x4x4x16-inner', (6, 4, 4, 16), [(2, 5)], 'q4 = 4 with an interior slab'),
    ('1x4x5x4', (1, 4, 5, 4), [(0, 1)], 'X = 1: no x neighbour at all'),
    ('6x1x1x4', (6, 1, 1, 4), [(0, 6)], 'Y = Z = 1: no y or z neighbour'),
]

# (id, step, grad_scale, tv_scale, lr, with tv_out)
HYPER = [
    ('step1', 1, 1.0, TV_SCALE, LR, True),            # bias corrections 0.1 and 0.01
    ('step100000', 100000, 1.0, TV_SCALE, LR, True),  # bias corrections 1 to float precision
    ('gscale', 7, 0.5, TV_SCALE, LR, True),
]
# one shape each (the three-slab one: every border kind): no TV term, so a voxel with grad = m = v = 0 has an exactly zero
# gradient; lr = 0, where p_out must be p_in bit for bit, run without a tv_out
HYPER_ONCE = [
    ('tv0', 3, 1.0, 0.0, LR, True),
    ('lr0-notv', 3, 1.0, TV_SCALE, 0.0, False),
]
ONCE_SHAPE = '13x5x3x8-slabs'

CHUNK_CASE = ((13, 5, 3, 8), (1, 12))
CHUNK_VALUES = [0, 1, 3, 11, 12, 4096]       # 12 and 4096 exceed nx = 11 and behave as 0

# (id, shape, slab, reason)
SPARSE_CASES = [
    ('13x5x3x8', (13, 5, 3, 8), (0, 13), 'whole grid: the prefetch of the next plane\'s marks ends at the grid'),
    ('13x5x3x8-inner', (13, 5, 3, 8), (4, 9), 'interior slab: marks and clears must stay inside it'),
    ('130x3x5x4-inner', (130, 3, 5, 4), (1, 129), '16 chunks of 8 planes, q4 = 1: every lane is a clearer'),
]


def sparse_inputs(shape, slab, seed=0):
    """grid_inputs plus a touched map [X,Y,Z] uint8 marking ~10 % of the voxels, among them one on the first and one on the last
    plane of the slab and one whose gradient is exactly 0; every unmarked voxel keeps its (mostly non-zero) gradient."""
    X, Y, Z, C = shape
    p, grad, m, v = grid_inputs(shape, seed)
    g = torch.Generator().manual_seed(2000 + seed)
    hit = torch.rand(X, Y, Z, generator=g) < 0.10
    xb, xe = slab
    hit[xb, 0, 0] = True
    hit[xe - 1, Y - 1, Z - 1] = True
    hit[xb + (xe - xb) // 2, Y // 2, Z // 2] = True
    grad[xb + (xe - xb) // 2, Y // 2, Z // 2] = 0.0
    return p, grad, m, v, hit.to(torch.uint8)


def serial_partial_sums(p, n_parts, n_orders=16):
    """float32 evaluations of tv_value(p) the way a pass with many work-groups adds it up: the terms are cut into n_parts
    consecutive pieces, each piece's sum is one float32 number, and these are added ONE AFTER THE OTHER onto a float32 total (one
    float atomic per work-group).  The atomics land in any order, so the evaluation is repeated for the natural order and
    n_orders - 1 seeded shuffles; the yardstick is the largest error among them.  Every step is a single IEEE float32 addition
    in a fixed order: the figures do not depend on the host."""
    p = p.double()
    own = torch.zeros_like(p)
    own[:-1] += (p[1:] - p[:-1]).abs()
    own[:, :-1] += (p[:, 1:] - p[:, :-1]).abs()
    own[:, :, :-1] += (p[:, :, 1:] - p[:, :, :-1]).abs()
    parts = np.array([float(c.sum()) for c in own.reshape(-1).tensor_split(n_parts)], dtype=np.float32)
    rng = np.random.RandomState(0)
    out = []
    for t in range(n_orders):
        total = np.float32(0)
        for i in (range(n_parts) if t == 0 else rng.permutation(n_parts)):
            total = np.float32(total + parts[i])
        out.append(float(total))
    return out


# ---- standalone TV ------------------------------------------------------------------------------------------------------
TV_SCALE_ARG, TV_GSCALAR = f32(0.37), 2.0
TV_SHAPES = sorted({c[1] for c in DENSE_CASES})                 # every dense shape, whole grid
# 130 tiles x 8 chunks = 1040 virtual blocks on a grid of 1024: the smallest shape at which the value pass loops twice
TV_VALUE_ONLY = [('8x105x105x12', (8, 105, 105, 12), 'persistent loop of the value pass takes a second pass')]
TV_VALUE_WORKGROUPS = 1024     # what the value pass runs at most; from there on its result is ~1000 partials added serially, and the
                               # yardstick of that shape is such a sum (kind 'tv.value.serial'), not the host's pairwise one
TV_ELEMENTWISE = [(5, 6, 7, 1), (5, 6, 7, 3), (5, 6, 7, 5)]      # C % 4 != 0: the element-wise gradient kernel


def tv_inputs(shape, seed=0):
    X, Y, Z, C = shape
    p = grid_inputs(shape, seed)[0]
    g = torch.Generator().manual_seed(3000 + seed)
    return p, torch.randn(X, Y, Z, C, generator=g)


# ---- flat Adam ----------------------------------------------------------------------------------------------------------
FLAT_N = [1, 255, 256, 257, 1000]
# five segments: one of a single element, an end on a block border (256), a frozen one, a last end short of n
FLAT_SEG_END = [1, 256, 257, 700, 900]
FLAT_SEG_LR = [f32(1e-1), 0.0, f32(1e-3), f32(1e-2), f32(1e-4)]
# (grad_scale, zero_grad, first step)
FLAT_HYPER = [(1.0, 1, 1), (0.25, 0, 1), (1.0, 0, 100000), (0.25, 1, 100000)]
FLAT_STEPS = 3


def flat_segments(n):
    """seg_end, seg_lr: the five-segment layout at n = 1000, one segment covering the buffer below."""
    return (FLAT_SEG_END, FLAT_SEG_LR) if n == 1000 else ([n], [f32(1e-2)])


def flat_inputs(n, seed=0):
    """p, m, v [n] and FLAT_STEPS gradients [FLAT_STEPS, n]; a few elements have grad = m = v = 0."""
    g = torch.Generator().manual_seed(4000 + seed + n)
    p = torch.randn(n, generator=g)
    m = torch.randn(n, generator=g) * 1e-2
    v = torch.rand(n, generator=g) * 1e-4
    grads = torch.randn(FLAT_STEPS, n, generator=g) * 1e-2
    zero = torch.arange(n) % 97 == 5
    m[zero], v[zero] = 0.0, 0.0
    grads[:, zero] = 0.0
    return p, m, v, grads


# ---- reference runs -----------------------------------------------------------------------------------------------------
def reference_dense(shape, slabs, hyper, dtype=torch.float64, seed=0):
    """The fused pass called slab after slab on one set of buffers -> (p_out, m, v, grad, tv) with p_out assembled from the
    slabs (p outside them) and tv the sum of the slabs' values."""
    from tests import optim_reference as R
    _, step, grad_scale, tv_scale, lr, _ = hyper
    p, grad, m, v = grid_inputs(shape, seed)
    p_out, tv = p.to(dtype).clone(), 0.0
    for xb, xe in slabs:
        po, m, v, grad, t = R.grid_step(p, grad, m, v, xb, xe, tv_scale, grad_scale, lr, B1, B2, EPS, step, dtype=dtype)
        p_out[xb:xe] = po[xb:xe]
        tv = tv + t
    return p_out, m, v, grad, tv


def dense_params():
    """(case, hyper) pairs of the dense fused pass."""
    out = [(c, h) for c in DENSE_CASES for h in HYPER]
    return out + [(c, h) for c in DENSE_CASES if c[0] == ONCE_SHAPE for h in HYPER_ONCE]


def reference_flat(n, hyper, dtype=torch.float64, seed=0):
    """FLAT_STEPS consecutive pp_adam_flat steps -> list of (p, m, v, grad_after) per step."""
    from tests import optim_reference as R
    grad_scale, zero_grad, step0 = hyper
    seg_end, seg_lr = flat_segments(n)
    p, m, v, grads = flat_inputs(n, seed)
    out = []
    for s in range(FLAT_STEPS):
        p, m, v, ga = R.adam_flat(p, grads[s], m, v, seg_end, seg_lr, grad_scale, B1, B2, EPS, step0 + s, zero_grad, dtype=dtype)
        out.append((p, m, v, ga))
    return out


def flat_segment_slices(n):
    seg_end, _ = flat_segments(n)
    edges = [0] + [min(e, n) for e in seg_end]
    return [slice(a, b if i < len(seg_end) - 1 else n) for i, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
