"""References of the k0 gradient scatter family (pp_k0_scatter_samples, pp_k0_pack_samples, pp_k0_scatter_packed and the
two sorted kernels), numpy and torch on the CPU only.

stencil32   the trilinear stencil of csrc/pp_k0_tri.h (pp_grid_u, k0_setup, k0_corner) restated in float32, one rounding per
            operation exactly as the device code does it (the library is built with -ffp-contract=off and uses __f*_rn).
replay32    the ordered float32 accumulation the sorted kernels promise: per voxel acc = 0; acc = acc + (w * g) in ascending
            (shard, sample, corner) order, then k0_grad[v] = prefill[v] + acc once.  Bit for bit what the kernels must give.
scatter64   the float64 answer, obtained WITHOUT the stencil: autograd of torch's grid_sample with respect to the feature grid.
pack_image  the expected byte image of pp_k0_pack_samples.
build_case  seeded sample sets that visit every way a sample can meet the grid border.

tests/test_scatter_reference.py checks these against each other before tests/test_hip_scatter_kernels.py trusts them.
"""
import itertools

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
XYZ_MIN = np.array([-0.6, -0.55, -0.7], np.float32)          # as in tests/test_hip_stage_kernels.py
XYZ_MAX = np.array([0.6, 0.5, 0.45], np.float32)
GRIDS = [(7, 4, 5), (2, 3, 2), (11, 6, 9)]
FEAT_LD = 64                                                  # row stride of the feature gradient (PP_FEAT_LD)
PACK_LD = 16                                                  # row length of the packed exchange format (PP_PACK_LD)
F32 = np.float32


class GridScene:
    """What the stencil needs of a scene: grid size and bounds."""

    def __init__(self, size, xyz_min=XYZ_MIN, xyz_max=XYZ_MAX):
        self.size = tuple(int(s) for s in size)
        self.mn = np.asarray(xyz_min, F32)
        self.mx = np.asarray(xyz_max, F32)
        self.n_voxels = int(np.prod(self.size))


def to_world(u, size):
    """Voxel coordinates [M,3] -> float32 world points (tests/test_hip_stage_kernels.py::to_world)."""
    size = np.asarray(size, np.float64)
    return (XYZ_MIN + np.asarray(u, np.float64) / (size - 1) * (XYZ_MAX - XYZ_MIN).astype(np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------------------------------ stencil
def stencil32(p, scene, F32=F32):
    """p [M,3] float32 -> dict(vox [M,8] flat voxel index (-1 outside), w [M,8] float32, ok [M,8], i0 [M,3], ok0 / ok1 [M,3]).
    Corner c: bit 4 -> x + 1, bit 2 -> y + 1, bit 1 -> z + 1; weight (wx * wy) * wz.
    F32=np.float64 evaluates the same formulas in float64 (only to find which voxels a sample reaches there, see replay32)."""
    p = np.ascontiguousarray(p, np.float32).astype(F32).reshape(-1, 3)
    M = len(p)
    size = np.array(scene.size, np.int64)
    w0, w1 = np.empty((M, 3), F32), np.empty((M, 3), F32)
    i0 = np.empty((M, 3), np.int64)
    with np.errstate(all='ignore'):
        for a in range(3):
            t = (p[:, a] - F32(scene.mn[a])) / (F32(scene.mx[a]) - F32(scene.mn[a]))   # pp_grid_u
            n = t * F32(2) - F32(1)
            u = ((n + F32(1)) / F32(2)) * F32(size[a] - 1)
            f = np.floor(u)                                                       # k0_setup
            w1[:, a] = u - f
            w0[:, a] = (f + F32(1)) - u
            fc = np.fmin(np.fmax(f, F32(-2)), F32(size[a]))                       # fmaxf / fminf: NaN -> -2
            i0[:, a] = fc.astype(np.int64)
        assert w0.dtype == w1.dtype == F32
        ok0 = (i0 >= 0) & (i0 < size)
        ok1 = (i0 + 1 >= 0) & (i0 + 1 < size)
        vox = np.full((M, 8), -1, np.int64)
        w = np.empty((M, 8), F32)
        ok = np.empty((M, 8), bool)
        for c in range(8):                                                        # k0_corner
            b = ((c >> 2) & 1, (c >> 1) & 1, c & 1)
            okc = np.ones(M, bool)
            for a in range(3):
                okc &= ok1[:, a] if b[a] else ok0[:, a]
            ix, iy, iz = i0[:, 0] + b[0], i0[:, 1] + b[1], i0[:, 2] + b[2]
            wa = [w1[:, a] if b[a] else w0[:, a] for a in range(3)]
            w[:, c] = (wa[0] * wa[1]) * wa[2]
            ok[:, c] = okc
            vox[okc, c] = ((ix * size[1] + iy) * size[2] + iz)[okc]
    return dict(vox=vox, w=w, ok=ok, i0=i0, ok0=ok0, ok1=ok1)


# ------------------------------------------------------------------------------------------------------------------- replay
def _pairs(shards, scene, C):
    """Valid (sample, corner) pairs of all shards in (shard, sample, corner) order: voxel [P], weight [P] f32, gradient rows
    [P,C] f32; and (voxel, gradient rows) of the pairs that exist in a float64 evaluation of the stencil only."""
    pts = np.concatenate([np.asarray(s[0], F32).reshape(-1, 3) for s in shards] + [np.zeros((0, 3), F32)])
    g = np.concatenate([np.asarray(s[1], F32)[:, :C] for s in shards] + [np.zeros((0, C), F32)])
    st = stencil32(pts, scene)
    ok = st['ok'].reshape(-1)
    sample = np.repeat(np.arange(len(pts)), 8)[ok]
    st64 = stencil32(pts, scene, np.float64)
    ok64 = st64['ok'].reshape(-1)
    sample64, vox64 = np.repeat(np.arange(len(pts)), 8)[ok64], st64['vox'].reshape(-1)[ok64]
    only64 = ~np.isin(sample64 * scene.n_voxels + vox64, sample * scene.n_voxels + st['vox'].reshape(-1)[ok])
    return st['vox'].reshape(-1)[ok], st['w'].reshape(-1)[ok], g[sample], vox64[only64], g[sample64[only64]]


def replay32(shards, scene, C, prefill):
    """shards: list of (pts [M,3], feat_grad [M,>=C]) holding the VALID samples only.  prefill [V,C] float32.
    Returns dict(grad [V,C] float32, n [V], A [V,C] float64 = sum |w g|, G [V,C] float64 = sum |g|, marks [V] bool).
    n, A and marks count the float32 pairs.  G is the budget of the weights' absolute error, so it also counts the pairs that
    exist in float64 only: a sample within rounding distance of a cell face reaches the voxel beyond the face in one precision
    and not in the other, with a weight of the order eps * size, which is the very error the G term of the bound stands for."""
    V = scene.n_voxels
    prefill = np.asarray(prefill)
    assert prefill.dtype == F32 and prefill.shape == (V, C)
    vox, w, g, vox64, g64 = _pairs(shards, scene, C)
    with np.errstate(all='ignore'):
        term = w[:, None] * g                                                     # pp_mul(w, g): one rounding
    assert term.dtype == F32
    n = np.bincount(vox, minlength=V)
    order = np.argsort(vox, kind='stable')                                        # per voxel: ascending pair order
    start = np.concatenate([[0], np.cumsum(n)])
    rank = np.empty(len(vox), np.int64)
    rank[order] = np.arange(len(vox)) - start[vox[order]]
    by_rank = np.argsort(rank, kind='stable')
    cut = np.searchsorted(rank[by_rank], np.arange(int(n.max(initial=0)) + 1))
    acc = np.zeros((V, C), F32)
    with np.errstate(all='ignore'):
        for k in range(len(cut) - 1):                                             # k-th contribution of every voxel at once
            sel = by_rank[cut[k]:cut[k + 1]]
            acc[vox[sel]] = acc[vox[sel]] + term[sel]
        marks = n > 0
        grad = prefill.copy()
        grad[marks] = prefill[marks] + acc[marks]
    A = np.zeros((V, C))
    G = np.zeros((V, C))
    np.add.at(A, vox, np.abs(term.astype(np.float64)))
    np.add.at(G, vox, np.abs(g.astype(np.float64)))
    np.add.at(G, vox64, np.abs(g64.astype(np.float64)))
    return dict(grad=grad, n=n, A=A, G=G, marks=marks)


# ------------------------------------------------------------------------------------------------------------------ float64
def scatter64(shards, scene, C):
    """[V,C] float64: d(sum_m <g_m, k0(p_m)>) / d k0 with k0(p) = grid_sample(k0, p, align_corners=True, zeros padding).
    Coordinates beyond 1e6 grid widths are pulled in to 1e6 (still far outside: they contribute nothing either way, and
    grid_sample's integer conversion stays defined).  Rows with non-finite coordinates must be removed by the caller."""
    X, Y, Z = scene.size
    pts = np.concatenate([np.asarray(s[0], F32).reshape(-1, 3) for s in shards] + [np.zeros((0, 3), F32)]).astype(np.float64)
    g = np.concatenate([np.asarray(s[1], F32)[:, :C] for s in shards] + [np.zeros((0, C), F32)])
    assert np.isfinite(pts).all()
    mn, mx = scene.mn.astype(np.float64), scene.mx.astype(np.float64)
    nrm = np.clip((pts - mn) / (mx - mn) * 2 - 1, -1e6, 1e6)
    k0 = torch.zeros(1, C, X, Y, Z, dtype=torch.float64, requires_grad=True)
    grid = torch.from_numpy(nrm[:, ::-1].copy()).reshape(1, -1, 1, 1, 3)          # grid_sample wants (z, y, x) for [.., X, Y, Z]
    out = torch.nn.functional.grid_sample(k0, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    up = torch.from_numpy(g.astype(np.float64).T.copy()).reshape(1, C, -1, 1, 1)
    out.backward(up)
    return k0.grad[0].permute(1, 2, 3, 0).reshape(X * Y * Z, C).numpy().copy()


# --------------------------------------------------------------------------------------------------------------------- pack
def pack_image(pts, feat_grad, count, capacity, C, before):
    """Expected [rows,16] float32 buffer after pp_k0_pack_samples into `before` (compare as int32 bit patterns)."""
    before = np.asarray(before)
    assert before.dtype == F32 and before.ndim == 2 and before.shape[1] == PACK_LD
    out = before.copy()
    M = max(0, min(int(count), int(capacity)))
    out[:M, :C] = np.asarray(feat_grad, F32)[:M, :C]
    out[:M, C:12] = 0
    out[:M, 12:15] = np.asarray(pts, F32)[:M]
    out[:M, 15] = 0
    out[0, 15:16].view(np.int32)[0] = M
    return out


def bits(x):
    """int32 view of a float32 array: equality of these is equality of bits (NaN payloads and -0.0 included)."""
    x = np.ascontiguousarray(x)
    assert x.dtype == F32
    return x.view(np.int32)


# -------------------------------------------------------------------------------------------------------------------- cases
N_CASE = 900
N_CELL = 64
CELL_AT = 100
# (count, capacity) of the GPU tests; the last pair clamps
COUNTS = [(0, 16), (1, 1), (15, 17), (16, 16), (17, 40), (255, 300), (257, 257), (700, 730), (900, 700)]
CORNER_PATTERNS = sorted(itertools.product(('lo', 'mid', 'hi'), repeat=3))       # per axis: only +1 in / both in / only +0 in


def axis_patterns(st):
    """Per sample the in/out state of each axis as a tuple of 'lo' (only the +1 plane inside), 'mid' (both), 'hi' (only the +0
    plane inside), 'out' (neither)."""
    name = np.where(st['ok0'] & st['ok1'], 'mid', np.where(st['ok1'], 'lo', np.where(st['ok0'], 'hi', 'out')))
    return [tuple(r) for r in name]


def build_case(size, seed=0):
    """900 sample positions for grid `size`, drawn in voxel coordinates.  Returns dict(pts [900,3] float32, kind [900] str,
    cell [64] = indices of the 64 samples that share one cell, in ascending order).  Sample 0 is an interior point."""
    size = np.asarray(size)
    rng = np.random.default_rng([seed, *size])
    hi = (size - 1).astype(np.float64)
    inside = lambda k: rng.uniform(0, 1, (k, 3)) * hi
    parts, kinds = [], []

    def add(kind, u=None, p=None):
        p = to_world(u, size) if p is None else p
        parts.append(p.astype(F32)); kinds.extend([kind] * len(p))

    add('interior', inside(388))
    add('node', np.floor(rng.uniform(0, 1, (60, 3)) * size))                      # exact lattice nodes
    for a in range(3):                                                            # the six faces: p = xyz_min / xyz_max exactly
        for side in (0, 1):
            p = to_world(inside(20), size)
            p[:, a] = (XYZ_MIN, XYZ_MAX)[side][a]
            add('face', p=p)
    for d in itertools.product((-1, 0, 1), repeat=3):                             # the one-voxel band outside every face
        if d == (0, 0, 0):
            continue
        u = inside(8)
        for a in range(3):
            if d[a]:
                band = rng.uniform(0.02, 0.98, 8)
                u[:, a] = -band if d[a] < 0 else hi[a] + band
        add('band', u)
    u = inside(40)                                                                # two or more voxels outside
    for r in range(40):
        a = rng.integers(3)
        off = rng.uniform(1.0, 6.0)
        u[r, a] = -1 - off if rng.integers(2) else hi[a] + 1 + off
    add('far', u)
    p = to_world(inside(20), size)                                                # finite, absurdly far
    for r in range(20):
        p[r, rng.integers(3)] = F32(1e30) if r % 2 else F32(-1e30)
    add('huge', p=p)
    pts, kind = np.concatenate(parts), np.array(kinds)
    perm = rng.permutation(len(pts))
    first = int(np.flatnonzero(kind[perm] == 'interior')[0])
    perm[[0, first]] = perm[[first, 0]]
    pts, kind = pts[perm], kind[perm]
    # row 8 carries a zero gradient (build_gradients): alone in the last cell among the first rows, it marks voxels that stay zero
    pts[8], kind[8] = to_world((size - 2 + rng.uniform(0.2, 0.8, 3))[None], size)[0], 'interior'
    # 64 samples in one cell, consecutive rows: every count from 255 up holds them all
    cell = to_world((size - 1) // 2 + rng.uniform(0.05, 0.95, (N_CELL, 3)), size)
    pts = np.concatenate([pts[:CELL_AT], cell, pts[CELL_AT:]])
    kind = np.concatenate([kind[:CELL_AT], ['cell'] * N_CELL, kind[CELL_AT:]])
    assert len(pts) == N_CASE
    return dict(pts=pts, kind=kind, cell=np.arange(CELL_AT, CELL_AT + N_CELL), size=tuple(int(s) for s in size))


def build_gradients(n, C, seed=0, junk=True):
    """[n,64] float32 feature-gradient rows: randn * exp(3 randn) per row, every ninth row (8, 17, ...) exactly zero (alternately -0
    and +0), a few single -0.0 entries.  Columns C..63 hold non-zero junk that no kernel may read."""
    rng = np.random.default_rng([seed, n, C])
    g = np.full((n, FEAT_LD), F32(3.0e4) if junk else F32(0), F32)
    g[:, :C] = (rng.standard_normal((n, C)) * np.exp(3 * rng.standard_normal((n, 1)))).astype(F32)
    g[8::9, :C] = 0
    g[8::18, :C] = -0.0
    rows = np.arange(4, n, 13)
    g[rows, rng.integers(0, C, len(rows))] = -0.0
    return g


def build_prefill(V, C, seed=0, scale=1.0):
    """[V,C] float32, seeded, no zero."""
    rng = np.random.default_rng([seed, V, C])
    p = (rng.standard_normal((V, C)) * scale).astype(F32)
    p[p == 0] = F32(scale)
    return p

