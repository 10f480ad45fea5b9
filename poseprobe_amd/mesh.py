"""Mesh extraction on the HIP path: the counterpart of the reference's `extract_geometry` chain (lib/dvgo_ori.py:679-703,
:381-396; lib/voxurf_coarse.py:1224-1263), with marching cubes as HIP kernels (csrc/pp_mesh.hip) instead of `mcubes`.

    from poseprobe_amd import mesh
    vertices, triangles = mesh.voxurf_extract_deform_geometry(model, bound_min, bound_max, resolution=512)
    mesh.write_ply('mesh.ply', vertices, triangles)

The field is sampled into a DEVICE lattice (no host copy per block), triangulated there, and only the finished mesh is
copied to the host.  Semantics of the triangulation (include/poseprobe_hip.h, DESIGN.md "Mesh extraction"): a corner is below
iff u < threshold, one vertex per sign-changing lattice edge, vertices and triangles in a canonical bit-reproducible order,
geometric normals toward decreasing u - for the reference's fields (u = -sdf, inside positive) the outward normal.  The
ordering and the winding of `mcubes` are not reproduced (neither can be observed offline); vertices are float32 where
`mcubes` returns float64.  Non-finite field values are the caller's problem.

The legacy names (`dvgo_ori.extract_geometry`, `DirectVoxGO.extract_geometry`, `Voxurf.extract_geometry`,
`Voxurf.extract_deform_geometry`) keep refusing; this module is the way to a mesh.
"""
import numpy as np
import torch

from . import ops
from .grid import channels_last_view


@torch.no_grad()
def marching_cubes(u, threshold):
    """u [X,Y,Z] fp32 on the device (a numpy array is uploaded; a CPU tensor is refused) -> (vertices [Nv,3] float32,
    triangles [Nt,3] int32), device tensors in lattice (index) coordinates.  One host read (the two counts) between the
    counting and the emitting pass."""
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).cuda()
    if not isinstance(u, torch.Tensor):
        raise TypeError('u must be a torch.Tensor or a numpy array')
    if not u.is_cuda:
        raise RuntimeError('u must be a CUDA tensor')
    if u.dim() != 3:
        raise RuntimeError('u must be a [X, Y, Z] lattice')
    u = u.detach().contiguous()
    dev = u.device
    with torch.cuda.device(dev):
        work = torch.empty(ops.mc_workspace(*u.shape), dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        ops.mc_count(u, threshold, work, counts)
        nv, nt = (int(c) for c in counts.tolist())
        if nt < 0:
            raise RuntimeError('marching_cubes: more than 2^31 - 1 triangles')
        vertices = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(nt, 3, dtype=torch.int32, device=dev)
        if nv > 0:                                  # (an empty surface launches nothing)
            ops.mc_emit(u, threshold, work, vertices, nv, triangles, nt)
    return vertices, triangles


@torch.no_grad()
def extract_fields_device(bound_min, bound_max, resolution, query_func, N=64, device='cuda'):
    """extract_fields (lib/dvgo_ori.py:679-693) with the lattice kept on the device: the same linspace axes and the same walk
    in blocks of N^3 points; query_func receives device points [n,3] and returns n device values."""
    resolution = int(resolution)
    axes = [torch.linspace(float(bound_min[a]), float(bound_max[a]), resolution).to(device) for a in range(3)]
    u = torch.empty([resolution] * 3, dtype=torch.float32, device=device)
    for x0 in range(0, resolution, N):
        for y0 in range(0, resolution, N):
            for z0 in range(0, resolution, N):
                xs, ys, zs = axes[0][x0:x0 + N], axes[1][y0:y0 + N], axes[2][z0:z0 + N]
                pts = torch.stack(torch.meshgrid(xs, ys, zs, indexing='ij'), dim=-1).reshape(-1, 3)
                u[x0:x0 + len(xs), y0:y0 + len(ys), z0:z0 + len(zs)] = query_func(pts).reshape(len(xs), len(ys), len(zs))
    return u


def _host(b):
    return (b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)).astype(np.float32)


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, N=64, device='cuda'):
    """lib/dvgo_ori.py:695-703 -> (vertices [Nv,3] in world coordinates, triangles [Nt,3] int32), numpy."""
    u = extract_fields_device(bound_min, bound_max, resolution, query_func, N, device)
    vertices, triangles = marching_cubes(u, threshold)
    b_min, b_max = _host(bound_min), _host(bound_max)
    vertices = vertices.cpu().numpy() / (int(resolution) - 1.0) * (b_max - b_min)[None, :] + b_min[None, :]
    return vertices, triangles.cpu().numpy()


def _resolution(model, resolution):
    return int(model.world_size[0]) if resolution is None else int(resolution)


def _lattice_scene(model, world_size, voxel_size=1.0, k0_dim=1, **kw):
    """pp_scene of a lookup on the model's box: only the box, the grid size (and, for the geometry kernel, the voxel size and the
    warp net's output range) matter - no rays are sampled."""
    return ops.make_scene(model.xyz_min.tolist(), model.xyz_max.tolist(), [int(v) for v in world_size], float(voxel_size), 1.0,
                          0., 1., 0., k0_dim=k0_dim, **kw)


def _grid_query(sc, grid_cl, border, sign):
    def query(pts):
        pts = pts.contiguous().float()
        out = torch.empty(pts.shape[0], 1, device=pts.device)
        ops.grid_sample_fwd(sc, grid_cl, 1, pts, border, out)
        return out[:, 0] * sign
    return query


def voxurf_field(model):
    """query_func of Voxurf.extract_geometry (lib/voxurf_coarse.py:1250-1256): grid_sampler(pts, -sdf.grid), border padding."""
    model.sdf.ensure_layout()
    grid = model.sdf.grid.detach()
    return _grid_query(_lattice_scene(model, grid.shape[2:]), channels_last_view(grid), 1, -1.0)


def voxurf_deform_field(model):
    """query_func of Voxurf.extract_deform_geometry (lib/voxurf_coarse.py:1224-1240): -(mapped sdf at the warped point +
    correction), evaluated by the kernels of the render path (pp_warp_fwd + pp_geometry_fwd) as Voxurf's surface-point query does."""
    grid = model.sdf.grid.detach()[0, 0].contiguous()
    dev = grid.device
    sc = _lattice_scene(model, grid.shape, model.voxel_size, model.k0_dim, out_range=model.warp_network.output_range)
    flat = model._flat_params(dev)
    ctx = getattr(model, 'pp_ctx', None)
    viewdir = torch.tensor([[0., 0., 1.]], device=dev)
    buf = {}

    def query(pts):
        pts = pts.contiguous().float()
        n = pts.shape[0]
        if buf.get('cap', 0) < n:
            buf.update(cap=n, acts=torch.empty(4, n * 4, 128, device=dev), warp=torch.empty(n, 16, device=dev),
                       ray_id=torch.zeros(n, dtype=torch.int32, device=dev), alpha=torch.empty(n, device=dev),
                       grad=torch.empty(n, 3, device=dev), count=torch.empty(1, dtype=torch.int32, device=dev))
        cap = buf['cap']
        if n < cap:                                 # the kernels index their buffers by the capacity they are given
            pts = torch.cat([pts, pts.new_zeros(cap - n, 3)])
        buf['count'].fill_(n)
        sdf_final = torch.empty(cap, device=dev)
        ops.warp_fwd(flat.view('warp'), pts, buf['count'], cap, sc.out_range, buf['acts'], buf['warp'], ctx)
        ops.geometry_fwd(sc, grid, flat.view('sdf_ab'), pts, buf['warp'], viewdir, buf['ray_id'], buf['count'], cap, 1.0,
                         buf['alpha'], buf['grad'], sdf_final, None, None)
        return -sdf_final[:n]
    return query


def voxurf_extract_geometry(model, bound_min, bound_max, resolution=128, threshold=0.0, **kwargs):
    """Voxurf.extract_geometry (lib/voxurf_coarse.py:1250-1263).  The reference's line reads `self.self.sdf.grid` and fails
    without smoothing; the evident intent (the raw template) is implemented.  Extra keyword arguments are ignored as the
    reference's **kwargs are."""
    return extract_geometry(bound_min, bound_max, _resolution(model, resolution), threshold, voxurf_field(model),
                            device=model.sdf.grid.device)


def voxurf_extract_deform_geometry(model, bound_min, bound_max, resolution=128, threshold=0.0, **kwargs):
    """Voxurf.extract_deform_geometry (lib/voxurf_coarse.py:1224-1248)."""
    return extract_geometry(bound_min, bound_max, _resolution(model, resolution), threshold, voxurf_deform_field(model),
                            device=model.sdf.grid.device)


def dvgo_field(model, mode='density'):
    """(query_func, threshold) of DirectVoxGO.extract_geometry (lib/dvgo_ori.py:381-389)."""
    if mode == 'density':
        grid = model.density.detach()[0, 0].contiguous()
        raw = _grid_query(_lattice_scene(model, grid.shape), grid[..., None], 0, 1.0)
        return (lambda pts: model.activate_density(raw(pts))), 0.001
    if mode == 'neus':
        if not hasattr(model, 'sdf'):
            raise NotImplementedError("mode='neus' reads `self.sdf`, which DirectVoxGO never creates (lib/dvgo_ori.py:386)")
        grid = torch.as_tensor(model.sdf).detach()[0, 0].contiguous()
        return _grid_query(_lattice_scene(model, grid.shape), grid[..., None], 0, -1.0), 0.0
    raise NameError(mode)


def dvgo_extract_geometry(model, bound_min, bound_max, resolution=128, threshold=0.0, mode='density', **kwargs):
    """DirectVoxGO.extract_geometry (lib/dvgo_ori.py:381-396): mode='density' forces the threshold 0.001, as the reference does."""
    query, threshold = dvgo_field(model, mode)
    return extract_geometry(bound_min, bound_max, _resolution(model, resolution), threshold, query, device=model.density.device)


def write_ply(path, vertices, triangles, vertex_colors=None):
    """Binary little-endian PLY: vertices [Nv,3] (stored as float32), triangles [Nt,3] (int32 lists of 3), optional
    vertex_colors [Nv,3] uint8 (or floats in [0,1]).  trimesh is not a dependency."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v = to_np(vertices).astype('<f4').reshape(-1, 3)
    t = to_np(triangles).astype('<i4').reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}', 'property float x', 'property float y',
              'property float z']
    if vertex_colors is not None:
        c = to_np(vertex_colors).reshape(-1, 3)
        if c.dtype != np.uint8:
            c = (255 * np.clip(c, 0, 1)).astype(np.uint8)
        if len(c) != len(v):
            raise ValueError('vertex_colors: one row per vertex')
        fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
        header += ['property uchar red', 'property uchar green', 'property uchar blue']
    header += [f'element face {len(t)}', 'property list uchar int vertex_indices', 'end_header']
    vert = np.empty(len(v), dtype=fields)
    vert['x'], vert['y'], vert['z'] = v[:, 0], v[:, 1], v[:, 2]
    if vertex_colors is not None:
        vert['red'], vert['green'], vert['blue'] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(t), dtype=[('n', 'u1'), ('v', '<i4', (3,))])
    face['n'], face['v'] = 3, t
    with open(path, 'wb') as f:
        f.write(('\n'.join(header) + '\n').encode('ascii'))
        f.write(vert.tobytes())
        f.write(face.tobytes())


_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def read_ply(path):
    """A minimal PLY reader: ascii and binary little-endian, scalar properties of the usual types, faces as lists of 3 vertex
    indices -> (vertices [Nv,3] in the stored float type, triangles [Nt,3] int32 - empty for a point cloud).  Other vertex
    properties (normals, colours) and other scalar-only elements are skipped.  It reads what `write_ply` writes."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError(f'{path}: not a PLY file')
    body = data.find(b'\n', end) + 1
    fmt, elements = None, []                    # elements: [name, count, [(property name, dtype or ('list', count type, item type))]]
    for line in data[:end].decode('ascii').splitlines()[1:]:
        w = line.split()
        if not w or w[0] in ('comment', 'obj_info'):
            continue
        if w[0] == 'format':
            fmt = w[1]
        elif w[0] == 'element':
            elements.append([w[1], int(w[2]), []])
        elif w[0] == 'property':
            if w[1] == 'list':
                elements[-1][2].append((w[4], ('list', _PLY_TYPES[w[2]], _PLY_TYPES[w[3]])))
            else:
                elements[-1][2].append((w[2], _PLY_TYPES[w[1]]))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError(f'{path}: format {fmt} is not supported (ascii and binary_little_endian are)')
    vertices, triangles = None, np.empty((0, 3), np.int32)
    tokens = data[body:].split() if fmt == 'ascii' else None
    pos = 0 if fmt == 'ascii' else body
    for name, count, props in elements:
        lists = [p for p in props if isinstance(p[1], tuple)]
        if lists and (name != 'face' or len(props) != 1):
            raise ValueError(f'{path}: element {name}: list properties are only read as the single property of `face`')
        if lists:
            ct, it = lists[0][1][1:]
            if fmt == 'ascii':
                rows = np.array(tokens[pos:pos + 4 * count], dtype=np.float64).reshape(count, 4)
                pos += 4 * count
                n, tri = rows[:, 0], rows[:, 1:]
            else:
                dt = np.dtype([('n', '<' + ct), ('v', '<' + it, (3,))])
                rows = np.frombuffer(data, dt, count, pos)
                pos += count * dt.itemsize
                n, tri = rows['n'], rows['v']
            if count and not (n == 3).all():
                raise ValueError(f'{path}: only triangle faces are read')
            triangles = np.ascontiguousarray(tri).astype(np.int32)
            continue
        dt = np.dtype([(p, '<' + t) for p, t in props])
        if fmt == 'ascii':
            rows = np.array(tokens[pos:pos + len(props) * count], dtype=np.float64).reshape(count, len(props))
            pos += len(props) * count
            col = {p: rows[:, k].astype(t) for k, (p, t) in enumerate(props)}
        else:
            rows = np.frombuffer(data, dt, count, pos)
            pos += count * dt.itemsize
            col = rows
        if name == 'vertex':
            vertices = np.stack([col['x'], col['y'], col['z']], -1)
    if vertices is None:
        raise ValueError(f'{path}: no vertex element')
    return vertices, triangles
