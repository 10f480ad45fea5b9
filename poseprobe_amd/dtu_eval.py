"""Mesh evaluation on the HIP path: the counterpart of the reference's lib/dtu_eval.py (the DTU Chamfer distance every reference
run ends with, run.py:94-130), with its three hot stages as HIP kernels (csrc/pp_dtu_eval.hip) on device-resident points.

    from poseprobe_amd import dtu_eval
    d2s, s2d, mean = dtu_eval.eval('mesh.ply', scene=122, eval_dir='out', dataset_dir='data/DTU')
    r = dtu_eval.chamfer(vertices, triangles, stl, obs_mask, bb, res, plane, runtime=True)     # arrays or tensors

    sample_mesh_points   lib/dtu_eval.py:70-89: the referenced vertices, then the points of every triangle; decided in float64 with
                         the reference's operation order, float32 on output
    thin_points          :98-106: the keep mask of the reference's loop in the given point order (`d2 <= radius^2`, inclusive)
    nearest              :145-146, :158-159: the exact nearest point; (inf, -1) beyond max_dist, which the reference drops from its
                         means anyway
Points are float32 and distances the float32 d2 = (dx dx + dy dy) + dz dz, where the reference works in float64 (DESIGN.md §18 has
the measured effect on the means).  Sorting, scans, masking, the observation-mask lookup and the means are torch plumbing.  The
shuffle in front of the thinning (:93-94) is the caller's - `perm` or `generator` - so every result is a pure function of its
inputs; without either a generator seeded with 0 is used.  The coloured error clouds of the reference are not written.
"""
import os

import numpy as np
import torch

from . import mesh, ops

PATCH = 60                   # lib/dtu_eval.py:40
MAX_CELLS = 1 << 13          # cells per axis of a neighbour grid: keeps the rounding of a cell coordinate below 2^-8 of a cell
EDGE_MARGIN = 1.01           # cell edge over the search radius: covers that rounding (csrc/pp_dtu_eval.hip)


def _dev(x, dtype, device='cuda'):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x))).to(device=device, dtype=dtype).contiguous()


def _points(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError(f'{name} must be a torch.Tensor')
    if not x.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor')
    if x.dim() != 2 or x.shape[1] != 3:
        raise RuntimeError(f'{name} must be [.,3]')
    if x.shape[0] > 2 ** 31 - 1:
        raise RuntimeError(f'{name}: more than 2^31 - 1 rows')
    return x.detach().float().contiguous()


@torch.no_grad()
def sample_mesh_points(vertices, triangles, thresh):
    """vertices [V,3] (any float type; used as float64), triangles [T,3] integer, device tensors -> float32 [N,3] on the device:
    the referenced vertices in index order, then the sampled points triangle-major, i-major, j-minor.  One host read (the total)."""
    if not (isinstance(vertices, torch.Tensor) and isinstance(triangles, torch.Tensor)):
        raise TypeError('vertices and triangles must be torch.Tensors')
    if not (vertices.is_cuda and triangles.is_cuda):
        raise RuntimeError('vertices and triangles must be CUDA tensors')
    v = vertices.detach().double().reshape(-1, 3).contiguous()
    t = triangles.detach().to(torch.int32).reshape(-1, 3).contiguous()
    V, T = v.shape[0], t.shape[0]
    if T == 0 or V == 0:
        return torch.empty(0, 3, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        lo, hi = int(t.min()), int(t.max())
        if lo < 0 or hi >= V:
            raise ValueError(f'triangles index vertices {lo}..{hi}, there are {V}')
        referenced = torch.zeros(V, dtype=torch.bool, device=v.device)
        referenced[t.reshape(-1).long()] = True
        counts = torch.empty(T, dtype=torch.int64, device=v.device)
        ops.dtu_sample_count(v, t, thresh, counts)
        ends = torch.cumsum(counts, 0)
        n = int(ends[-1])
        kept = v[referenced].float()
        if n + kept.shape[0] > 2 ** 31 - 1:
            raise RuntimeError('sample_mesh_points: more than 2^31 - 1 points')
        out = torch.empty(kept.shape[0] + n, 3, dtype=torch.float32, device=v.device)
        out[:kept.shape[0]] = kept
        if n > 0:
            ops.dtu_sample_emit(v, t, thresh, (ends - counts).contiguous(), out[kept.shape[0]:], n)
    return out


class _Cells:
    """points [N,3] float32 (N >= 1) sorted into a sparse grid of cubic cells with edge >= min_edge: .points, .keys (ascending
    int64), .order (int32: index before sorting), .grid = (origin, edge, cells)."""

    def __init__(self, points, min_edge):
        lo, hi = points.min(0).values.tolist(), points.max(0).values.tolist()
        if not all(np.isfinite(lo + hi)):
            raise ValueError('non-finite point coordinates')
        extent = max(h - l for l, h in zip(lo, hi))
        edge = float(np.float32(max(float(min_edge), extent / (MAX_CELLS - 2), 1e-30)))
        cells = [min(int((h - l) / edge) + 1, MAX_CELLS) for l, h in zip(lo, hi)]
        self.grid = (lo, edge, cells)
        keys = torch.empty(points.shape[0], dtype=torch.int64, device=points.device)
        ops.dtu_cell_keys(points, self.grid, keys)
        self.keys, perm = torch.sort(keys, stable=True)
        self.points = points[perm].contiguous()
        self.order = perm.to(torch.int32)


@torch.no_grad()
def thin_points(points, radius, info=None):
    """points [N,3] on the device -> bool keep mask [N]: walk the points in order; a point still marked keeps itself and unmarks
    every point with d2 <= radius^2.  Computed in rounds (one host read per batch of rounds); info (a dict) receives `rounds`."""
    p = _points(points, 'points')
    N = p.shape[0]
    keep = torch.zeros(N, dtype=torch.bool, device=p.device)
    if info is not None:
        info['rounds'] = 0
    if N == 0:
        return keep
    radius = float(np.float32(radius))
    if not (radius >= 0 and np.isfinite(radius)):
        raise ValueError('radius must be non-negative and finite')
    with torch.cuda.device(p.device):
        cells = _Cells(p, np.float32(radius) * np.float32(EDGE_MARGIN))
        work = torch.empty(ops.dtu_thin_workspace(N), dtype=torch.uint8, device=p.device)
        flags = torch.empty(256, dtype=torch.int32, device=p.device)
        done, batch = 0, 4
        while True:
            ops.dtu_thin_rounds(cells.points, cells.keys, cells.order, cells.grid, radius, done, batch, work, flags)
            left = flags[:batch].tolist()
            if left[-1] == 0:
                rounds = done + left.index(0) + 1
                done += batch
                break
            done += batch
            batch = min(2 * batch, 256)
        keep[cells.order.long()] = ops.dtu_thin_state(work, N, done) == 1
    if info is not None:
        info['rounds'] = rounds
    return keep


@torch.no_grad()
def nearest(queries, points, max_dist, *, cell_edge=None):
    """queries [Q,3], points [P,3] on the device -> (d2 float32 [Q], idx int32 [Q]): the exact nearest point by float32 d2, ties to
    the lowest index; (inf, -1) where no point has d2 < max_dist^2.  cell_edge is the edge of the internal search grid (default
    max_dist / 16); the result does not depend on it."""
    q, p = _points(queries, 'queries'), _points(points, 'points')
    max_dist = float(np.float32(max_dist))
    if not (max_dist > 0 and np.isfinite(max_dist)):
        raise ValueError('max_dist must be positive and finite')
    if cell_edge is not None and not (cell_edge > 0 and np.isfinite(cell_edge)):
        raise ValueError('cell_edge must be positive and finite')
    Q, P = q.shape[0], p.shape[0]
    d2 = torch.full((Q,), float('inf'), dtype=torch.float32, device=q.device)
    idx = torch.full((Q,), -1, dtype=torch.int32, device=q.device)
    if P == 0 or Q == 0:
        return d2, idx
    with torch.cuda.device(q.device):
        cells = _Cells(p, max_dist / 16 if cell_edge is None else cell_edge)
        ops.dtu_nearest(q, cells.points, cells.keys, cells.order, cells.grid, max_dist, d2, idx)
    return d2, idx


def _mean(d2):
    d = d2[torch.isfinite(d2)].double().sqrt()
    return float(d.mean()) if d.numel() else float('nan')


@torch.no_grad()
def chamfer(vertices, triangles, stl, obs_mask, bb, res, plane, *, max_dist=20, runtime=False, perm=None, generator=None,
            scale_mat=None, device='cuda'):
    """lib/dtu_eval.py:37-160 on arrays or tensors: vertices [V,3], triangles [T,3], stl [S,3] (the scanned cloud), obs_mask
    [X,Y,Z], bb [2,3], res (scalar), plane [4] -> dict(mean_d2s, mean_s2d, over_all (floats: means in float64 over sqrt(d2)),
    n_sampled, n_down, n_in_obs, n_stl_above).  scale_mat [4,4] applies v s[0,0] + s[:3,3] first (run.py:107-108).  perm (a
    permutation of the n_sampled points) or generator (for torch.randperm) is the shuffle in front of the thinning."""
    v = _dev(vertices, torch.float64, device).reshape(-1, 3)
    t = _dev(triangles, torch.int32, device).reshape(-1, 3)
    if scale_mat is not None:
        s = _dev(scale_mat, torch.float64, device)
        v = v * s[0, 0] + s[:3, 3][None]
    thresh = 0.5 if runtime else 0.2
    pcd = sample_mesh_points(v, t, thresh)
    if perm is None:
        if generator is None:
            generator = torch.Generator().manual_seed(0)
        perm = torch.randperm(pcd.shape[0], generator=generator, device=generator.device)
    perm = _dev(perm, torch.int64, device).reshape(-1)
    if perm.numel() != pcd.shape[0]:
        raise ValueError(f'perm has {perm.numel()} entries, {pcd.shape[0]} points were sampled')
    pcd = pcd[perm]
    down = pcd[thin_points(pcd, thresh)]

    bb = _dev(bb, torch.float32, device).reshape(2, 3)
    inbound = ((down >= bb[:1] - PATCH) & (down < bb[1:] + PATCH * 2)).sum(-1) == 3
    data_in = down[inbound]
    obs = _dev(obs_mask, torch.bool, device)
    res = _dev(res, torch.float64, device).reshape(-1)[0]
    grid = torch.round((data_in.double() - bb[:1].double()) / res).long()          # (half to even, as np.around)
    shape = torch.tensor(obs.shape, device=grid.device)
    grid_inbound = ((grid >= 0) & (grid < shape[None])).sum(-1) == 3
    g = grid[grid_inbound]
    data_in_obs = data_in[grid_inbound][obs[g[:, 0], g[:, 1], g[:, 2]]]

    stl = _dev(stl, torch.float32, device).reshape(-1, 3)
    if runtime:
        num_gt = data_in_obs.shape[0] * 2
        stl = stl[::max(stl.shape[0] // num_gt if num_gt else 1, 1)].contiguous()
    d2s, _ = nearest(data_in_obs, stl, max_dist)
    P = [float(x) for x in np.asarray(plane.detach().cpu() if isinstance(plane, torch.Tensor) else plane, np.float64).reshape(4)]
    s64 = stl.double()
    above = ((P[0] * s64[:, 0] + P[1] * s64[:, 1]) + P[2] * s64[:, 2]) + P[3] > 0
    stl_above = stl[above]
    s2d, _ = nearest(stl_above, data_in, max_dist)
    m1, m2 = _mean(d2s), _mean(s2d)
    return dict(mean_d2s=m1, mean_s2d=m2, over_all=(m1 + m2) / 2, n_sampled=int(pcd.shape[0]), n_down=int(down.shape[0]),
                n_in_obs=int(data_in_obs.shape[0]), n_stl_above=int(stl_above.shape[0]))


def eval(in_file, scene, eval_dir, dataset_dir='data/DTU', suffix='', max_dist=20, use_o3d=False, runtime=False, **kw):
    """lib/dtu_eval.py::eval: reads the mesh, {dataset_dir}/Points/stl/stl{scene:03}_total.ply, ObsMask/ObsMask{scene}_10.mat and
    ObsMask/Plane{scene}.mat, writes {eval_dir}/result{suffix}.txt and returns (mean_d2s, mean_s2d, over_all).  use_o3d is
    accepted and ignored; perm / generator / device pass through to `chamfer`."""
    from scipy.io import loadmat
    scene = int(scene)
    vertices, triangles = mesh.read_ply(in_file)
    stl, _ = mesh.read_ply(f'{dataset_dir}/Points/stl/stl{scene:03}_total.ply')
    obs_file = loadmat(f'{dataset_dir}/ObsMask/ObsMask{scene}_10.mat')
    plane = loadmat(f'{dataset_dir}/ObsMask/Plane{scene}.mat')['P']
    r = chamfer(vertices, triangles, stl, obs_file['ObsMask'], obs_file['BB'], np.asarray(obs_file['Res'], np.float64), plane,
                max_dist=max_dist, runtime=runtime, **kw)
    with open(f'{eval_dir}/result{suffix}.txt', 'w') as f:
        f.write(f'{r["mean_d2s"]} {r["mean_s2d"]} {r["over_all"]}')
    return r['mean_d2s'], r['mean_s2d'], r['over_all']


def validate_mesh(model, cfg, resolution=128, threshold=0.0, prefix='', world_space=False, scale_mats_np=None, gt_eval=False,
                  runtime=True, scene=122, extract_color=False, keep=None, **kw):
    """run.py:94-131: extract the mesh of `model` on its box, write {cfg.basedir}/{cfg.expname}/meshes/{scene}_{prefix}.ply and,
    with gt_eval, score it: -> over_all (0.0 without gt_eval).  keep (None: every component, else as mesh.keep_components:
    'largest', a triangle count or a fraction of the largest) drops connected components on the device before the mesh is
    written and scored.  Extra keyword arguments (smooth, ...) are ignored."""
    if extract_color:
        raise NotImplementedError('validate_mesh: extract_color=True (vertex colours from the colour net) is not implemented')
    vertices, triangles = mesh.voxurf_extract_geometry(model, model.xyz_min.detach().float(), model.xyz_max.detach().float(),
                                                       resolution=resolution, threshold=threshold, keep=keep)
    if world_space and scale_mats_np is not None:
        vertices = vertices * scale_mats_np[0, 0] + scale_mats_np[:3, 3][None]
    mesh_dir = os.path.join(cfg.basedir, cfg.expname, 'meshes')
    os.makedirs(mesh_dir, exist_ok=True)
    mesh_path = os.path.join(mesh_dir, '{}_'.format(scene) + prefix + '.ply')
    mesh.write_ply(mesh_path, vertices, triangles)
    if gt_eval:
        return eval(mesh_path, scene=scene, eval_dir=mesh_dir, dataset_dir='data/DTU', suffix=prefix + 'eval', runtime=runtime)[2]
    return 0.


def validate_deform_mesh(model, cfg, resolution=128, threshold=0.0, prefix='', world_space=False, scale_mats_np=None, gt_eval=False,
                         extract_color=False, scene=122, runtime=True, keep=None, **kw):
    """lib/recon_scene.py:846-875, the export the training loop ends its object phase with (:748-751): extract the DEFORMED mesh
    of `model` on its box (mesh.voxurf_extract_deform_geometry), with extract_color shade every vertex through the colour net
    (mesh.voxurf_vertex_colors on the UNSCALED vertices, the normal direction as the view direction), apply the world_space
    transform and write {cfg.basedir}/{cfg.expname}/meshes/deform{prefix}.ply.  With gt_eval the file is scored as
    validate_mesh scores its own (-> over_all); 0.0 otherwise.  keep (None: every component, else as mesh.keep_components) drops
    connected components on the device right after the extraction: only the kept vertices are shaded, written and scored.  Of the
    extra keyword arguments, use_deform / global_step / chunk go to the colour pass; the rest (smooth, ...) is ignored."""
    vertices0, triangles = mesh.voxurf_extract_deform_geometry(model, model.xyz_min.detach().float(), model.xyz_max.detach().float(),
                                                               resolution=resolution, threshold=threshold, keep=keep)
    colors = None
    if extract_color:
        color_kw = {k: kw[k] for k in ('use_deform', 'global_step', 'chunk') if k in kw}
        colors = mesh.voxurf_vertex_colors(model, vertices0, **color_kw)
    vertices = vertices0
    if world_space and scale_mats_np is not None:
        vertices = vertices0 * scale_mats_np[0, 0] + scale_mats_np[:3, 3][None]
    mesh_dir = os.path.join(cfg.basedir, cfg.expname, 'meshes')
    os.makedirs(mesh_dir, exist_ok=True)
    mesh_path = os.path.join(mesh_dir, 'deform' + prefix + '.ply')
    mesh.write_ply(mesh_path, vertices, triangles, vertex_colors=colors)
    if gt_eval:
        return eval(mesh_path, scene=scene, eval_dir=mesh_dir, dataset_dir='data/DTU', suffix=prefix + 'eval', runtime=runtime)[2]
    return 0.
