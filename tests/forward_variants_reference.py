"""Torch restatement of the two branches of the reference's Voxurf.forward / Voxurf.inference beside the default one, in the dtype
of its inputs (float64 for the kernel tests, float32 for the yardstick of their tolerance):

  * plain_geometry: use_deform=False (lib/voxurf_coarse.py:986-989 with neus_sdf_gradient :458-467 and
    neus_alpha_from_sdf_scatter :483-519) - the mapped grid and the 3-channel grid of its central differences ARE built here,
    and sampled with F.grid_sample as grid_sampler does (:528-541);
  * threshold_mask / keep: fast_color_thres (:996-1003, :1144-1151).

tests/test_forward_variants_host.py compares both with a recorded run of the reference (tests/golden/forward_variants_g24.npz,
written by tools/make_forward_variants_golden.py), tests/test_hip_forward_variants.py compares the kernels with them."""
import numpy as np
import torch
import torch.nn.functional as F

CASES = ('plain', 'thres', 'plain_thres')          # fixture cases: use_deform=False | fast_color_thres=1e-3 | both
CASE_SWITCHES = {'plain': (False, 0.0), 'thres': (True, 1e-3), 'plain_thres': (False, 1e-3)}   # (use_deform, fast_color_thres)
RENDER_KWARGS = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, inverse_y=True, flip_x=False, flip_y=False)
GRAD_ROW_STEP = 4           # the fixture stores every 4th row of an MLP weight gradient (all rows of a matrix with fewer than 4)


def flat_params(P):
    """The tensors of an oracle parameter dict in a fixed order."""
    return [P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta']] + [t for net in ('rgbnet', 'warp') for Wb in P[net] for t in Wb]


def fixture_params(d):
    """The fixture's parameters, regenerated from its seed as the tool generated them (they are not stored: 0.7 MB of noise),
    in the 'P.*' layout of the forward_*.npz fixtures; checked against the stored checksums."""
    from oracle import voxurf_oracle as O
    from tests.helpers import scene_for
    P = O.init_params(scene_for(int(d['G'])), seed=int(d['seed']))
    P['sdf_alpha'] = torch.tensor([float(d['sdf_alpha'])])          # the tool's one change to the seeded set (its setup())
    sums = np.array([float(v.double().abs().sum()) for v in flat_params(P)])
    assert np.allclose(sums, d['P.checksum'], rtol=1e-12, atol=0), 'the regenerated parameters are not the recorded ones'
    out = {'P.k0': P['k0'].numpy(), 'P.sdf': P['sdf'].numpy(), 'P.sdf_alpha': P['sdf_alpha'].numpy(), 'P.sdf_beta': P['sdf_beta'].numpy()}
    for net in ('rgbnet', 'warp'):
        for li, (Wt, b) in enumerate(P[net]):
            out[f'P.{net}.{li}.weight'], out[f'P.{net}.{li}.bias'] = Wt.numpy(), b.numpy()
    return out


def mapped_grid(sdf, sdf_alpha, sdf_beta):
    """sdf [X,Y,Z] -> softplus10(alpha) (sigmoid(softplus10(beta) sdf) - 0.5)   (:947-949)."""
    sp = lambda t: F.softplus(t, beta=10)
    return sp(sdf_alpha) * (torch.sigmoid(sp(sdf_beta) * sdf) - 0.5)


def central_differences(G, voxel_size):
    """neus_sdf_gradient(mode='interpolate') of G [X,Y,Z] -> [3,X,Y,Z]; a component is zero on the boundary planes of its axis."""
    g = torch.zeros((3,) + tuple(G.shape), dtype=G.dtype, device=G.device)
    g[0, 1:-1, :, :] = (G[2:, :, :] - G[:-2, :, :]) / 2 / voxel_size
    g[1, :, 1:-1, :] = (G[:, 2:, :] - G[:, :-2, :]) / 2 / voxel_size
    g[2, :, :, 1:-1] = (G[:, :, 2:] - G[:, :, :-2]) / 2 / voxel_size
    return g


def grid_sample(grid, pts, xyz_min, xyz_max):
    """grid_sampler's F.grid_sample route (:528, :540-541): grid [C,X,Y,Z], pts [M,3] -> [M,C]."""
    ind = ((pts - xyz_min) / (xyz_max - xyz_min)).flip((-1,)) * 2 - 1
    out = F.grid_sample(grid[None], ind.reshape(1, 1, 1, -1, 3), mode='bilinear', align_corners=True, padding_mode='border')
    return out.reshape(grid.shape[0], -1).T


def neus_alpha(dirs, dist, sdf, gradient, inv_s):
    """neus_alpha_from_sdf_scatter, use_mid, cos_anneal_ratio = 1; dirs [M,3] = viewdirs[ray_id]."""
    true_cos = (dirs * gradient).sum(-1, keepdim=True)
    iter_cos = -F.relu(-true_cos)
    sdf = sdf.unsqueeze(-1)
    nxt = sdf + iter_cos * dist * 0.5
    prv = sdf - iter_cos * dist * 0.5
    prev_cdf, next_cdf = torch.sigmoid(prv * inv_s), torch.sigmoid(nxt * inv_s)
    return (((prev_cdf - next_cdf) + 1e-5) / (prev_cdf + 1e-5)).clip(0.0, 1.0).squeeze(-1)


def plain_geometry(sdf, sdf_alpha, sdf_beta, pts, dirs, xyz_min, xyz_max, voxel_size, dist, inv_s):
    """-> sdf_final [M], gradient [M,3], alpha [M].  Every tensor in one dtype; voxel_size, dist, inv_s python floats or 0-d tensors."""
    G = mapped_grid(sdf, sdf_alpha, sdf_beta)
    sdf_final = grid_sample(G[None], pts, xyz_min, xyz_max)[:, 0]
    gradient = grid_sample(central_differences(G, voxel_size), pts, xyz_min, xyz_max)
    return sdf_final, gradient, neus_alpha(dirs, dist, sdf_final, gradient, inv_s)


def threshold_mask(weights, thres):
    return weights > thres


def margin_to_threshold(weights, thres):
    """Smallest relative distance of a weight from the threshold: the mask of two fp32 implementations is the same set when this
    exceeds their relative error on a weight."""
    w = np.asarray(weights, dtype=np.float64)
    return float(np.abs(w - thres).min() / thres) if w.size else np.inf


# ------------------------------------------------------------------------------------------------- inputs of the kernel tests
def kernel_case(shape, seed):
    """A small template with its box, and points that exercise every path of the plain-geometry kernels: interior points of cells
    picked at random - boundary cells of every axis included by construction (cells 0 and size - 2 of each axis are always drawn) -,
    points ON cell faces (one, two or three lattice coordinates), the eight box corners, and points on the box's faces.  Cells are
    0.25 wide, so lattice points are exact in fp32.  -> dict of float64 tensors / python values; `lattice` [M] marks the points
    with at least one lattice coordinate (where the interpolant's derivative jumps)."""
    g = torch.Generator().manual_seed(seed)
    X, Y, Z = shape
    size = torch.tensor([X, Y, Z], dtype=torch.float64)
    h = 0.25
    xyz_min = torch.tensor([-0.5, 0.25, -1.0], dtype=torch.float64)
    xyz_max = xyz_min + (size - 1) * h
    sdf = (torch.rand(X, Y, Z, generator=g, dtype=torch.float64) - 0.5) * 1.2
    cells = []
    for a, n in enumerate(shape):                       # every boundary cell pair (first, last) of every axis, crossed with random others
        for edge in (0, n - 2):
            for _ in range(6):
                c = [int(torch.randint(0, m - 1, (1,), generator=g)) for m in shape]
                c[a] = edge
                cells.append(c)
    for _ in range(40):
        cells.append([int(torch.randint(0, m - 1, (1,), generator=g)) for m in shape])
    cells = torch.tensor(cells, dtype=torch.float64)
    frac = torch.rand(cells.shape[0], 3, generator=g, dtype=torch.float64) * 0.9 + 0.05
    interior = xyz_min + (cells + frac) * h
    # lattice points: some coordinates on cell faces (interior and box faces), the rest inside a cell
    n_lat = 48
    node = torch.stack([torch.randint(0, m, (n_lat,), generator=g) for m in shape], -1).double()
    inside = torch.stack([torch.randint(0, m - 1, (n_lat,), generator=g) for m in shape], -1).double() \
        + torch.rand(n_lat, 3, generator=g, dtype=torch.float64) * 0.9 + 0.05
    on_face = torch.rand(n_lat, 3, generator=g) < 0.5
    on_face[torch.arange(n_lat), torch.randint(0, 3, (n_lat,), generator=g)] = True        # at least one lattice coordinate each
    faces = xyz_min + torch.where(on_face, node, inside) * h
    corners = torch.tensor([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=torch.float64)
    corners = xyz_min + corners * (size - 1) * h
    pts = torch.cat([interior, faces, corners], 0)
    lattice = torch.cat([torch.zeros(interior.shape[0], dtype=torch.bool), torch.ones(n_lat + 8, dtype=torch.bool)])
    M = pts.shape[0]
    n_rays = 7
    ray_id = torch.sort(torch.randint(0, n_rays, (M,), generator=g)).values
    viewdirs = F.normalize(torch.randn(n_rays, 3, generator=g, dtype=torch.float64), dim=-1)
    return dict(shape=shape, sdf=sdf, xyz_min=xyz_min, xyz_max=xyz_max, voxel_size=float(np.float32(h)), stepsize=1.5,
                inv_s=float(np.float32(1.0) / np.float32(0.2)), sdf_alpha=torch.tensor([1.3], dtype=torch.float64),
                sdf_beta=torch.tensor([0.9], dtype=torch.float64), pts=pts, lattice=lattice, ray_id=ray_id, viewdirs=viewdirs,
                n_rays=n_rays, g_alpha=torch.randn(M, generator=g, dtype=torch.float64),
                g_gradient=torch.randn(M, 3, generator=g, dtype=torch.float64) * 0.1)


def kernel_case_reference(case, dtype):
    """plain_geometry and the gradients of sum(g_alpha alpha) + sum(g_gradient gradient) in `dtype` -> dict of float64 numpy arrays:
    sdf_final, gradient, alpha, g_pts, g_view (per sample: d / d viewdirs[ray_id]), g_ab [2]."""
    c = lambda t: t.detach().clone().to(dtype)
    pts = c(case['pts']).requires_grad_(True)
    dirs = c(case['viewdirs'])[case['ray_id']].requires_grad_(True)
    a, b = c(case['sdf_alpha']).requires_grad_(True), c(case['sdf_beta']).requires_grad_(True)
    dist = torch.tensor(np.float32(case['stepsize']) * np.float32(case['voxel_size']), dtype=dtype)
    sdf_final, gradient, alpha = plain_geometry(c(case['sdf']), a, b, pts, dirs, c(case['xyz_min']), c(case['xyz_max']),
                                                torch.tensor(case['voxel_size'], dtype=dtype), dist,
                                                torch.tensor(case['inv_s'], dtype=dtype))
    ((c(case['g_alpha']) * alpha).sum() + (c(case['g_gradient']) * gradient).sum()).backward()
    n = lambda t: t.detach().double().numpy()
    return dict(sdf_final=n(sdf_final), gradient=n(gradient), alpha=n(alpha), g_pts=n(pts.grad), g_view=n(dirs.grad),
                g_ab=np.array([float(a.grad), float(b.grad)]))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def bound(r32, r64, floor_ulps=4):
    """This project's convention for a kernel against a float64 restatement: 4 x the largest error of the same restatement run in
    float32, but at least `floor_ulps` float32 ulps of the largest magnitude (the kernel's results are float32 themselves)."""
    r32, r64 = np.asarray(r32, np.float64), np.asarray(r64, np.float64)
    if r64.size == 0:
        return 0.0
    return max(4 * float(np.abs(r32 - r64).max()), floor_ulps * ulp32(float(np.abs(r64).max())))
