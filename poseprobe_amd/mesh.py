"""Mesh extraction on the HIP path: the counterpart of the reference's `extract_geometry` chain (lib/dvgo_ori.py:679-703,
:381-396; lib/voxurf_coarse.py:1224-1263), with marching cubes as HIP kernels (csrc/pp_mesh.hip) instead of `mcubes`.

    from poseprobe_amd import mesh
    vertices, triangles = mesh.voxurf_extract_deform_geometry(model, bound_min, bound_max, resolution=512)
    mesh.write_ply('mesh.ply', vertices, triangles)
    attr = mesh.vertex_attributes(model, vertices)          # unit normals and colours on the device (csrc/pp_mesh_color.hip)
    mesh.write_ply('mesh.ply', vertices, triangles, vertex_colors=attr['colors'], vertex_normals=attr['normals'])
    kept = mesh.keep_components(vertices, triangles, keep='largest', attributes=attr)     # drop the floaters (csrc/pp_mesh_components.hip)
    mesh.write_ply('clean.ply', kept['vertices'], kept['triangles'], vertex_colors=kept['colors'], vertex_normals=kept['normals'])

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


def extract_geometry(bound_min, bound_max, resolution, threshold, query_func, N=64, device='cuda', keep=None):
    """lib/dvgo_ori.py:695-703 -> (vertices [Nv,3] in world coordinates, triangles [Nt,3] int32), numpy.  keep (None: everything,
    else as keep_components) drops connected components on the device, before the mesh is copied to the host."""
    u = extract_fields_device(bound_min, bound_max, resolution, query_func, N, device)
    vertices, triangles = marching_cubes(u, threshold)
    if keep is not None:
        kept = keep_components(vertices, triangles, keep)
        vertices, triangles = kept['vertices'], kept['triangles']
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


def voxurf_extract_geometry(model, bound_min, bound_max, resolution=128, threshold=0.0, keep=None, **kwargs):
    """Voxurf.extract_geometry (lib/voxurf_coarse.py:1250-1263).  The reference's line reads `self.self.sdf.grid` and fails
    without smoothing; the evident intent (the raw template) is implemented.  keep as extract_geometry; the other extra keyword
    arguments are ignored as the reference's **kwargs are."""
    return extract_geometry(bound_min, bound_max, _resolution(model, resolution), threshold, voxurf_field(model),
                            device=model.sdf.grid.device, keep=keep)


def voxurf_extract_deform_geometry(model, bound_min, bound_max, resolution=128, threshold=0.0, keep=None, **kwargs):
    """Voxurf.extract_deform_geometry (lib/voxurf_coarse.py:1224-1248); keep as extract_geometry."""
    return extract_geometry(bound_min, bound_max, _resolution(model, resolution), threshold, voxurf_deform_field(model),
                            device=model.sdf.grid.device, keep=keep)


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


SHIPPED_COLOR_STAGE = dict(k0_dim=12, posbase_pe=5, viewbase_pe=1, rgbnet_width=128)


def _color_stage_config(model):
    """The SceneConfig of the model's box and colour stage (its pp_scene, its BARF weights); refuses what pp_vertex_feat does not cover."""
    from .engine import SceneConfig
    kw = getattr(model, 'rgbnet_kwargs', {})
    got = dict(k0_dim=int(getattr(model, 'k0_dim', -1)), posbase_pe=kw.get('posbase_pe'), viewbase_pe=kw.get('viewbase_pe'),
               rgbnet_width=kw.get('rgbnet_width'))
    if got != SHIPPED_COLOR_STAGE:
        raise NotImplementedError(f'vertex colours cover the shipped colour stage {SHIPPED_COLOR_STAGE} only, the model has {got}')
    cfg = SceneConfig(model.xyz_min.cpu().numpy(), model.xyz_max.cpu().numpy(), int(model.num_voxels), N_iters=model.N_iters,
                      barf_c2f=None if model.barf_c2f is None else tuple(model.barf_c2f), posbase_pe=got['posbase_pe'],
                      viewbase_pe=got['viewbase_pe'], k0_dim=got['k0_dim'], out_range=model.warp_network.output_range)
    if list(cfg.world_size) != [int(s) for s in model.sdf.grid.shape[2:]]:
        raise RuntimeError(f'the sdf template is {tuple(model.sdf.grid.shape[2:])}, num_voxels gives {cfg.world_size}')
    return cfg


def _device_vertices(vertices, dev):
    if isinstance(vertices, np.ndarray):
        vertices = torch.from_numpy(np.array(vertices, dtype=np.float32)).to(dev)       # (a copy: the array may be read-only)
    if not isinstance(vertices, torch.Tensor):
        raise TypeError('vertices must be a torch.Tensor or a numpy array')
    if not vertices.is_cuda:
        raise RuntimeError('vertices must be a CUDA tensor')
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError('vertices must be [Nv, 3]')
    return vertices.detach().to(device=dev, dtype=torch.float32).contiguous()


@torch.no_grad()
def vertex_attributes(model, vertices, use_deform=True, global_step=None, chunk=262144):
    """Normals and colours of mesh vertices on the device: the colour stage of the render path with every vertex seen head-on
    (the reference's drivers call a `mesh_color_forward` that its Voxurf does not define).  vertices [Nv,3] in MODEL
    coordinates (before any world_space scaling): a numpy array is uploaded, a CPU tensor is refused.
        g = d sdf / d p        the render path's `gradient`: through the warp net (use_deform=True) or the plain template's
                               interpolated central differences (use_deform=False)
        normal = g / (|g| + 1e-5), viewdir = -normal
        rgb = sigmoid(rgbnet([k0(p) | PE(p) | PE(viewdir) | normal]))
    The BARF weights follow the model's stored `progress` (global_step=None) or global_step / N_iters; nothing of the model is
    written.  Three launches per chunk of `chunk` vertices (pp_warp_fwd, pp_vertex_feat, pp_rgbnet_fwd, no activations kept);
    buffers are allocated once, for min(chunk, Nv) rows; every row is computed on its own, so the result does not depend on `chunk`.
    -> dict(normals [Nv,3], colors [Nv,3] in [0,1]), float32 on the device."""
    dev = model.sdf.grid.device
    v = _device_vertices(vertices, dev)
    cfg = _color_stage_config(model)
    if not use_deform:
        model._check_template_mode(False)
    chunk = int(chunk)
    if chunk <= 0:
        raise ValueError('chunk must be positive')
    Nv = v.shape[0]
    f = dict(dtype=torch.float32, device=dev)
    normals, colors = torch.empty(Nv, 3, **f), torch.empty(Nv, 3, **f)
    if Nv == 0:
        return dict(normals=normals, colors=colors)
    progress = float(model.progress.detach()) if global_step is None else global_step / model.N_iters
    with torch.cuda.device(dev):
        pe_w = torch.from_numpy(cfg.pe_weights(progress)).to(dev)
        model.k0.ensure_layout()
        k0_cl = channels_last_view(model.k0.grid.detach())
        sdf = model.sdf.grid.detach()[0, 0].contiguous()
        flat = model._flat_params(dev)
        ctx = getattr(model, 'pp_ctx', None)
        from . import _lib
        octx = _lib.default_context() if ctx is None else ctx
        split = octx.get('mlp_split') if octx.get('mlp_fused') else 0       # forward-only MLP calls: the split-precision kernels (the default)
        cap = min(chunk, Nv)
        pts = torch.zeros(cap, 3, **f)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        warp_out = torch.empty(cap, 16, **f) if use_deform else None
        warp_acts = None if (split & 1 or not use_deform) else torch.empty(4, cap * 4, 128, **f)
        rgb_acts = None if split & 4 else torch.empty(3, cap, 128, **f)
        feat, rgb = torch.empty(cap, ops.FEAT_LD, **f), torch.empty(cap, 3, **f)
        for at in range(0, Nv, cap):
            n = min(cap, Nv - at)
            pts[:n] = v[at:at + n]
            count.fill_(n)
            if use_deform:
                ops.warp_fwd(flat.view('warp'), pts, count, cap, cfg.out_range, warp_acts, warp_out, ctx)
            ops.vertex_feat(cfg.pp, sdf, flat.view('sdf_ab'), k0_cl, pts, warp_out, pe_w, n, normals[at:at + n], feat)
            ops.rgbnet_fwd(flat.view('rgbnet'), feat, count, cap, rgb_acts, rgb, ctx)
            colors[at:at + n] = rgb[:n]
    return dict(normals=normals, colors=colors)


def voxurf_vertex_colors(model, vertices, **kw):
    """The loop the reference's export drivers run over `model.mesh_color_forward` (lib/recon_scene.py:859-866): colours [Nv,3] in
    [0,1] of the vertices, on the device; keyword arguments as vertex_attributes."""
    return vertex_attributes(model, vertices, **kw)['colors']


CC_BATCH = 4                 # rounds of the labelling per host read
CC_MAX_BATCHES = 64          # batches before connected_components gives up (DESIGN.md §15.2 has the reasoning behind both)


def _mesh_triangles(triangles, n_vertices, device=None):
    """triangles [Nt,3] -> contiguous int32 on the device, every index inside [0, n_vertices).  A numpy array (any integer type)
    is checked on the host and uploaded; a device tensor must be int32 and costs one reduction and one host read; a CPU tensor is
    refused.  Type, dtype and shape are looked at before the device is."""
    Nv = int(n_vertices)
    if Nv < 0:
        raise ValueError('n_vertices must not be negative')
    if Nv > 2 ** 30:
        raise ValueError('at most 2^30 vertices')
    is_np = isinstance(triangles, np.ndarray)
    if not (is_np or isinstance(triangles, torch.Tensor)):
        raise TypeError('triangles must be a torch.Tensor or a numpy array')
    if is_np and not np.issubdtype(triangles.dtype, np.integer):
        raise TypeError(f'triangles must hold integers, got {triangles.dtype}')
    if not is_np and triangles.dtype != torch.int32:
        raise TypeError(f'triangles must be torch.int32, got {triangles.dtype}')
    if triangles.ndim != 2 or triangles.shape[1] != 3:
        raise ValueError(f'triangles must be [Nt, 3], got {tuple(triangles.shape)}')
    if triangles.shape[0] > 2 ** 29:
        raise ValueError('at most 2^29 triangles')
    if not is_np and not triangles.is_cuda:
        raise RuntimeError('triangles must be a CUDA tensor')
    if triangles.shape[0] > 0:
        if is_np:
            lo, hi = int(triangles.min()), int(triangles.max())
        else:
            lo, hi = torch.stack(torch.aminmax(triangles.detach())).tolist()
        if lo < 0 or hi >= Nv:
            raise ValueError(f'triangles index vertices {lo}..{hi}, there are {Nv}')
    if is_np:
        return torch.from_numpy(np.array(triangles, dtype=np.int32)).to('cuda' if device is None else device)   # (a copy: the array may be read-only)
    return triangles.detach().contiguous()


@torch.no_grad()
def connected_components(triangles, n_vertices, info=None):
    """Connected components of an indexed mesh on the device (csrc/pp_mesh_components.hip): two vertices are
    connected when some triangle contains both.  triangles [Nt,3] int32 on the device (a numpy array is uploaded); an index outside
    [0, n_vertices) is a ValueError before anything runs.
    -> dict(labels [Nv] int32: the smallest vertex index of the vertex's component, -1 for a vertex no triangle references;
            roots [C] int32 ascending: the components' labels; vertex_counts [C], triangle_counts [C] int32: their referenced
            vertices and triangles; n_components: C, an int), tensors on the device.
    The labelling runs in rounds (hook + jump), CC_BATCH rounds per host read; info (a dict) receives `rounds`, the rounds up to
    and including the first one that changed nothing - a pure function of the mesh, like the labels.  RuntimeError after
    CC_MAX_BATCHES batches without a fixpoint."""
    return _connected_components(_mesh_triangles(triangles, n_vertices), int(n_vertices), info)


def _connected_components(t, Nv, info):
    """connected_components on triangles _mesh_triangles has checked (keep_components checks once and comes here)."""
    Nt, dev = t.shape[0], t.device
    if info is not None:
        info['rounds'] = 0
    i32 = dict(dtype=torch.int32, device=dev)
    labels = torch.empty(Nv, **i32)
    empty = torch.empty(0, **i32)
    if Nv == 0:
        return dict(labels=labels, roots=empty, vertex_counts=empty.clone(), triangle_counts=empty.clone(), n_components=0)
    with torch.cuda.device(dev):
        work = torch.empty(ops.cc_workspace(Nv), dtype=torch.uint8, device=dev)
        changed = torch.empty(CC_BATCH, **i32)
        rounds = 0
        if Nt == 0:
            ops.cc_rounds(t, Nv, 0, 1, labels, work, changed)          # initialises: every label -1, no round to run
        else:
            done = 0
            while rounds == 0:
                if done >= CC_BATCH * CC_MAX_BATCHES:
                    raise RuntimeError(f'connected_components: labels still changing after {done} rounds '
                                       f'({CC_MAX_BATCHES} batches of {CC_BATCH}); {Nv} vertices, {Nt} triangles')
                ops.cc_rounds(t, Nv, done, CC_BATCH, labels, work, changed)
                moved = changed.tolist()
                if 0 in moved:
                    rounds = done + moved.index(0) + 1
                done += CC_BATCH
        by_root_v, by_root_t = torch.empty(Nv, **i32), torch.empty(Nv, **i32)
        ops.cc_count(labels, t, by_root_v, by_root_t)
        roots = torch.nonzero(by_root_v > 0).reshape(-1)                # a root is referenced and counts itself
        out = dict(labels=labels, roots=roots.to(torch.int32), vertex_counts=by_root_v[roots], triangle_counts=by_root_t[roots],
                   n_components=int(roots.numel()))
    if info is not None:
        info['rounds'] = rounds
    return out


def _check_keep(keep):
    if isinstance(keep, str):
        if keep != 'largest':
            raise ValueError(f"keep: unknown rule '{keep}' ('largest', an int or a float in (0, 1))")
    elif isinstance(keep, bool) or not isinstance(keep, (int, float, np.integer, np.floating)):
        raise TypeError(f"keep must be 'largest', an int or a float in (0, 1), got {type(keep).__name__}")
    elif isinstance(keep, (int, np.integer)):
        if keep < 0:
            raise ValueError('keep: a minimum triangle count must not be negative')
    elif not 0.0 < keep < 1.0:
        raise ValueError(f'keep: a fraction must lie in (0, 1), got {keep}')


@torch.no_grad()
def keep_components(vertices, triangles, keep='largest', attributes=None, info=None):
    """Drop connected components of a mesh on the device.  vertices [Nv,3], triangles [Nt,3] int32 (device tensors, or numpy arrays
    that are uploaded).  keep:
        'largest'           the component with the most triangles, ties to the lowest root
        an int              every component with at least that many triangles
        a float in (0, 1)   every component with at least that fraction of the largest component's triangle count
                            (float64: count >= keep * largest)
    -> dict(vertices [Nv',3] float32, triangles [Nt',3] int32, vertex_index [Nv'] int32: each kept vertex's old index,
            n_components: before the filter, n_kept: after), plus `attributes` - a dict of [Nv, ...] tensors or arrays - subset
    with vertex_index under the same keys.  Kept vertices and triangles stay in their relative order and the winding is untouched;
    vertices no triangle references are dropped.  Host reads: the index check (device triangles only), one per batch of rounds, the
    number of roots (torch.nonzero) and one for the kept counts.  info as connected_components'."""
    _check_keep(keep)
    dev = next((x.device for x in (vertices, triangles) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device('cuda'))
    if not isinstance(vertices, (torch.Tensor, np.ndarray)):
        raise TypeError('vertices must be a torch.Tensor or a numpy array')
    if not (vertices.is_floating_point() if isinstance(vertices, torch.Tensor) else np.issubdtype(vertices.dtype, np.floating)):
        raise TypeError(f'vertices must hold floats, got {vertices.dtype}')
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError(f'vertices must be [Nv, 3], got {tuple(vertices.shape)}')
    Nv = len(vertices)
    attributes = {} if attributes is None else dict(attributes)
    for k, a in attributes.items():
        if k in ('vertices', 'triangles', 'vertex_index', 'n_components', 'n_kept'):
            raise ValueError(f'attributes: the key {k!r} is one of the result\'s own')
        if not isinstance(a, (torch.Tensor, np.ndarray)) or a.ndim < 1 or a.shape[0] != Nv:
            raise ValueError(f'attributes[{k!r}] must be a tensor or an array with one row per vertex ({Nv})')
    t = _mesh_triangles(triangles, Nv, dev)
    v = _device_vertices(vertices, dev)
    cc = _connected_components(t, Nv, info)
    C, Nt = cc['n_components'], t.shape[0]
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        tcount = cc['triangle_counts']
        if C == 0:
            keep_c = torch.zeros(0, dtype=torch.bool, device=dev)
        elif isinstance(keep, str):
            keep_c = tcount == tcount.max()
            keep_c &= torch.cumsum(keep_c, 0) == 1                      # ties: the lowest root
        elif isinstance(keep, (int, np.integer)):
            keep_c = tcount >= int(keep)
        else:
            keep_c = tcount.double() >= float(keep) * tcount.max().double()
        root_keep = torch.zeros(Nv, dtype=torch.uint8, device=dev)
        root_keep[cc['roots'][keep_c].long()] = 1
        vkeep, tkeep = torch.empty(Nv, **i32), torch.empty(Nt, **i32)
        ops.cc_keep_masks(cc['labels'], t, root_keep, vkeep, tkeep)
        vscan, tscan = torch.cumsum(vkeep, 0, dtype=torch.int32), torch.cumsum(tkeep, 0, dtype=torch.int32)
        zero = torch.zeros(1, **i32)
        nv, nt, n_kept = torch.cat([vscan[-1:] if Nv else zero, tscan[-1:] if Nt else zero, keep_c.sum().to(torch.int32)[None]]).tolist()
        out_v, out_i, out_t = torch.empty(nv, 3, dtype=torch.float32, device=dev), torch.empty(nv, **i32), torch.empty(nt, 3, **i32)
        ops.cc_compact(v, t, vscan, tscan, out_v, out_i, out_t)
        out = dict(vertices=out_v, triangles=out_t, vertex_index=out_i, n_components=C, n_kept=n_kept)
        index = out_i.long()
        for k, a in attributes.items():
            out[k] = a[index.cpu().numpy()] if isinstance(a, np.ndarray) else a[index.to(a.device)]
    return out


def write_ply(path, vertices, triangles, vertex_colors=None, vertex_normals=None):
    """Binary little-endian PLY: vertices [Nv,3] (stored as float32), triangles [Nt,3] (int32 lists of 3), optional
    vertex_normals [Nv,3] (stored as float32 nx ny nz) and vertex_colors [Nv,3] uint8 (or floats in [0,1]).  trimesh is not a
    dependency."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v = to_np(vertices).astype('<f4').reshape(-1, 3)
    t = to_np(triangles).astype('<i4').reshape(-1, 3)
    fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
    header = ['ply', 'format binary_little_endian 1.0', f'element vertex {len(v)}', 'property float x', 'property float y',
              'property float z']
    if vertex_normals is not None:
        nrm = to_np(vertex_normals).astype('<f4').reshape(-1, 3)
        if len(nrm) != len(v):
            raise ValueError('vertex_normals: one row per vertex')
        fields += [('nx', '<f4'), ('ny', '<f4'), ('nz', '<f4')]
        header += ['property float nx', 'property float ny', 'property float nz']
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
    if vertex_normals is not None:
        vert['nx'], vert['ny'], vert['nz'] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
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


def _read_ply(path):
    """-> (columns of the vertex element by property name, triangles [Nt,3] int32 - empty for a point cloud)."""
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
    vertex, triangles = None, np.empty((0, 3), np.int32)
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
            vertex = {p: col[p] for p, _ in props}
    if vertex is None:
        raise ValueError(f'{path}: no vertex element')
    return vertex, triangles


def read_ply(path):
    """A minimal PLY reader: ascii and binary little-endian, scalar properties of the usual types, faces as lists of 3 vertex
    indices -> (vertices [Nv,3] in the stored float type, triangles [Nt,3] int32 - empty for a point cloud).  Other vertex
    properties (normals, colours: read_ply_attributes returns them) and other scalar-only elements are skipped.  It reads what
    `write_ply` writes."""
    col, triangles = _read_ply(path)
    return np.stack([col['x'], col['y'], col['z']], -1), triangles


def read_ply_attributes(path):
    """read_ply with the vertex attributes: -> dict(vertices [Nv,3], triangles [Nt,3] int32, normals [Nv,3] (nx ny nz) or None,
    colors [Nv,3] (red green blue, in the stored type: uint8 as write_ply writes them) or None)."""
    col, triangles = _read_ply(path)
    group = lambda names: np.stack([col[n] for n in names], -1) if all(n in col for n in names) else None
    return dict(vertices=group(('x', 'y', 'z')), triangles=triangles, normals=group(('nx', 'ny', 'nz')),
                colors=group(('red', 'green', 'blue')))


# ------------------------------------------------------------------------------------------- mesh -> signed distance grid
MSDF_MAX_CELLS = 1 << 13     # cells per axis of the triangle grid: keeps the rounding of a cell coordinate below 2^-8 of a cell
MSDF_CELLS_ACROSS = 48       # the default cell edge is at least the mesh's longest extent over this


def _check_points(x, name):
    """x [N,3]: a float numpy array or a float device tensor; type, dtype and shape are looked at before the device is."""
    if not isinstance(x, (torch.Tensor, np.ndarray)):
        raise TypeError(f'{name} must be a torch.Tensor or a numpy array')
    if not (x.is_floating_point() if isinstance(x, torch.Tensor) else np.issubdtype(x.dtype, np.floating)):
        raise TypeError(f'{name} must hold floats, got {x.dtype}')
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError(f'{name} must be [N, 3], got {tuple(x.shape)}')
    if isinstance(x, torch.Tensor) and not x.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor')


def _mesh_on_device(vertices, triangles):
    """(vertices float32 [Nv,3], triangles int32 [Nt,3]) on one device; an index out of range is a ValueError.  Everything that can
    be refused without the device is refused before the first upload."""
    _check_points(vertices, 'vertices')
    dev = next((x.device for x in (vertices, triangles) if isinstance(x, torch.Tensor) and x.is_cuda), torch.device('cuda'))
    t = _mesh_triangles(triangles, len(vertices), dev)
    return _device_vertices(vertices, dev), t


class _TriangleCells:
    """The triangles of a mesh registered in a sparse grid of cubic cells over the mesh's bounding box (pp_msdf_bin_*): .keys
    (ascending int64), .tris (int32), .grid = (origin, edge, cells).  Two host reads: the bounding box with the mean triangle
    area, and the pair total."""

    def __init__(self, v, t, cell_edge=None):
        used = v[t.reshape(-1).long()].reshape(-1, 3, 3)
        area = 0.5 * torch.linalg.cross(used[:, 1] - used[:, 0], used[:, 2] - used[:, 0]).norm(dim=-1).double().mean()
        lo, hi = used.amin((0, 1)), used.amax((0, 1))
        *box, area = torch.cat([lo.double(), hi.double(), area[None]]).tolist()
        if not all(np.isfinite(box)):
            raise ValueError('non-finite vertex coordinates')
        lo, hi = box[:3], box[3:]
        extent = max(h - l for l, h in zip(lo, hi))
        if cell_edge is None:                       # about two triangles across a cell, and no more cells than a far query can walk
            cell_edge = max(2.0 * np.sqrt(area) if np.isfinite(area) else 0.0, extent / MSDF_CELLS_ACROSS)
        edge = float(np.float32(max(float(cell_edge), extent / (MSDF_MAX_CELLS - 2), 1e-30)))
        cells = [min(int((h - l) / edge) + 1, MSDF_MAX_CELLS) for l, h in zip(lo, hi)]
        self.grid = (lo, edge, cells)
        counts = torch.empty(t.shape[0], dtype=torch.int64, device=v.device)
        ops.msdf_bin_count(v, t, self.grid, counts)
        ends = torch.cumsum(counts, 0)
        self.n_pairs = int(ends[-1])
        if self.n_pairs > 2 ** 31 - 1:
            raise RuntimeError(f'{self.n_pairs} (cell, triangle) pairs: more than 2^31 - 1; use a larger cell_edge than {edge}')
        keys = torch.empty(self.n_pairs, dtype=torch.int64, device=v.device)
        tris = torch.empty(self.n_pairs, dtype=torch.int32, device=v.device)
        ops.msdf_bin_emit(v, t, self.grid, (ends - counts).contiguous(), keys, tris, self.n_pairs)
        self.keys, perm = torch.sort(keys, stable=True)
        self.tris = tris[perm].contiguous()


def _max_dist(max_dist):
    if max_dist is None:
        return float('inf')
    max_dist = float(np.float32(max_dist))
    if not max_dist > 0:
        raise ValueError('max_dist must be positive')
    return max_dist


def _nearest_on_mesh(queries, axes, v, t, max_dist, cell_edge, info):
    dev = v.device
    Q = queries.shape[0] if queries is not None else int(np.prod([a.numel() for a in axes]))
    dist = torch.full((Q,), float('inf'), dtype=torch.float32, device=dev)
    closest = torch.full((Q, 3), float('nan'), dtype=torch.float32, device=dev)
    tri = torch.full((Q,), -1, dtype=torch.int32, device=dev)
    if info is not None:
        info.update(cell_edge=None, cells=None, pairs=0, rings_mean=0.0, rings_max=0)
    if Q == 0 or t.shape[0] == 0:
        return dist, closest, tri
    if Q > 2 ** 31 - 1:
        raise ValueError('more than 2^31 - 1 queries')
    with torch.cuda.device(dev):
        cells = _TriangleCells(v, t, cell_edge)
        rings = torch.empty(Q, dtype=torch.int32, device=dev) if info is not None else None
        ops.msdf_nearest(queries, axes, v, t, cells.keys, cells.tris, cells.grid, max_dist, dist, closest, tri, rings)
        if info is not None:
            info.update(cell_edge=cells.grid[1], cells=list(cells.grid[2]), pairs=cells.n_pairs,
                        rings_mean=float(rings.double().mean()), rings_max=int(rings.max()))
    return dist, closest, tri


@torch.no_grad()
def unsigned_distance(points, vertices, triangles, max_dist=None, *, cell_edge=None, info=None):
    """The exact distance from points [Q,3] to a triangle mesh on the device (csrc/pp_mesh_sdf.hip): vertices
    [Nv,3], triangles [Nt,3]; every input a numpy array (uploaded) or a device tensor.
    -> (dist [Q] float32, closest [Q,3] float32: the nearest point of the mesh, triangle [Q] int32: the triangle it lies on),
    device tensors.  float32 arithmetic; among triangles at the same float32 squared distance the lowest index wins, so the result
    is a pure function of the inputs - and does not depend on cell_edge, the edge of the internal search grid.  Triangles without
    area take part as segments or points.  max_dist (optional) caps the search: (inf, NaN, -1) where nothing is nearer.  An
    index outside the vertices is a ValueError.  info (a dict) receives cell_edge, cells, pairs (the (cell, triangle) pairs sorted),
    rings_mean and rings_max (rings of cells a query visited)."""
    _check_points(points, 'points')
    v, t = _mesh_on_device(vertices, triangles)
    return _nearest_on_mesh(_device_vertices(points, v.device), None, v, t, _max_dist(max_dist), cell_edge, info)


def sdf_grid_axes(xyz_min, xyz_max, world_size):
    """The node coordinates of a grid: node i of axis a sits at xyz_min[a] + i (xyz_max[a] - xyz_min[a]) / (world_size[a] - 1),
    formed in float64 and rounded once -> three float32 numpy vectors.  (world_size 1: the single node sits at xyz_min.)"""
    f64 = lambda b: np.asarray(b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b, dtype=np.float64).reshape(3)
    lo, hi = f64(xyz_min), f64(xyz_max)             # (the values as given: a float32 box is taken exactly)
    n = [int(s) for s in (world_size.tolist() if isinstance(world_size, (torch.Tensor, np.ndarray)) else world_size)]
    if len(n) != 3 or min(n) < 1:
        raise ValueError(f'world_size must be three positive counts, got {n}')
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError('xyz_min and xyz_max must be finite with xyz_min < xyz_max')
    axes = [(lo[a] + np.arange(n[a], dtype=np.float64) * ((hi[a] - lo[a]) / max(n[a] - 1, 1))).astype(np.float32) for a in range(3)]
    if any(len(x) > 1 and not (np.diff(x) > 0).all() for x in axes):
        raise ValueError('the float32 node coordinates are not strictly increasing: the grid is too fine for the box')
    return axes


def odd_edge_count(triangles):
    """The number of undirected edges with an odd number of incident triangles (a triangle that repeats a vertex contributes its
    sides as they are).  triangles [Nt,3] int on the device -> int (one host read).  0 is the condition under which the parity of
    crossings is the same along every generic line, i.e. under which inside and outside are defined."""
    t = triangles.long()
    if t.shape[0] == 0:
        return 0
    e = torch.cat([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    e = e[e[:, 0] != e[:, 1]]                       # (a side from a vertex to itself is no edge)
    if e.shape[0] == 0:
        return 0
    key = e.amin(1) * (int(t.max()) + 1) + e.amax(1)
    _, counts = torch.unique(key, return_counts=True)
    return int((counts % 2 == 1).sum())


@torch.no_grad()
def signed_distance_grid(vertices, triangles, xyz_min, xyz_max, world_size, check=True, info=None, *, cell_edge=None):
    """The signed distance of a closed triangle mesh at the nodes of a grid, on the device (csrc/pp_mesh_sdf.hip):
    the inverse of marching_cubes.  -> [X,Y,Z] float32, NEGATIVE inside, as the cuboid template and voxurf_field's -sdf have it.
    Node (i,j,k) sits at xyz_min + (i,j,k) (xyz_max - xyz_min) / (world_size - 1) (sdf_grid_axes), where params_init.cube_sdf's
    np.mgrid puts it.  The magnitude is unsigned_distance's; a node is inside iff the line through it along x crosses the mesh an
    odd number of times before it - independent of the triangles' winding, so a reversed inner shell is a cavity.
    Indices out of range are a ValueError.  check=True also refuses with ValueError non-finite vertices and a mesh in which some
    undirected edge has an odd number of incident triangles (the message counts them) - the condition under which the parity is
    defined: it admits the 4-triangle edges marching cubes can produce and rejects a surface cut open by the box.  check=False
    computes whatever the counting gives.  info as unsigned_distance's."""
    axes_np = sdf_grid_axes(xyz_min, xyz_max, world_size)
    v, t = _mesh_on_device(vertices, triangles)
    dev = v.device
    if check:
        if not bool(torch.isfinite(v).all()):
            raise ValueError('signed_distance_grid: non-finite vertex coordinates')
        odd = odd_edge_count(t)
        if odd:
            raise ValueError(f'signed_distance_grid: {odd} edges have an odd number of incident triangles: the mesh is not closed, '
                             'so inside and outside are not defined (check=False computes the crossing parity anyway)')
    X, Y, Z = (len(a) for a in axes_np)
    if t.shape[0] == 0 or v.shape[0] == 0:
        raise ValueError('signed_distance_grid: the mesh has no triangles')
    with torch.cuda.device(dev):
        axes = tuple(torch.from_numpy(a).to(dev) for a in axes_np)
        dist, _, _ = _nearest_on_mesh(None, axes, v, t, float('inf'), cell_edge, info)
        counts = torch.empty(ops.msdf_crossing_slots(X, Y, Z), dtype=torch.int32, device=dev)
        ops.msdf_crossings(v, t, *axes, counts)
        inside = (torch.cumsum(counts.view(X + 1, Y, Z)[:X], 0, dtype=torch.int32) & 1).bool()
        dist = dist.view(X, Y, Z)
        return torch.where(inside, -dist, dist)


def save_sdf_grid(path, sdf, xyz_min, xyz_max):
    """Write a template in the format the reference's MaskCache reads (lib/voxurf_coarse.py:1271-1282): a pickled dict with
    sdf_grid_xyz [X,Y,Z] float32, xyz_min [3] and xyz_max [3] (numpy arrays)."""
    import pickle
    g = sdf.detach().cpu().numpy() if isinstance(sdf, torch.Tensor) else np.asarray(sdf)
    g = np.ascontiguousarray(g.reshape(g.shape[-3:]), dtype=np.float32)
    if g.ndim != 3:
        raise ValueError('sdf must be [X,Y,Z] (or [1,1,X,Y,Z])')
    with open(path, 'wb') as f:
        pickle.dump({'sdf_grid_xyz': g, 'xyz_min': _host(xyz_min).reshape(3), 'xyz_max': _host(xyz_max).reshape(3)}, f)


def load_sdf_grid(path):
    """-> (sdf [X,Y,Z] float32, xyz_min [3], xyz_max [3]), numpy: what save_sdf_grid wrote.  The file is a pickle: load only files
    you trust."""
    import pickle
    with open(path, 'rb') as f:
        d = pickle.load(f)
    if not isinstance(d, dict) or not all(k in d for k in ('sdf_grid_xyz', 'xyz_min', 'xyz_max')):
        raise ValueError(f'{path}: not a template file (a dict with sdf_grid_xyz, xyz_min, xyz_max)')
    g = np.asarray(d['sdf_grid_xyz'], dtype=np.float32)
    if g.ndim != 3:
        raise ValueError(f'{path}: sdf_grid_xyz must be [X,Y,Z], got {g.shape}')
    return g, np.asarray(d['xyz_min'], np.float32).reshape(3), np.asarray(d['xyz_max'], np.float32).reshape(3)


@torch.no_grad()
def voxurf_template_from_mesh(model, vertices, triangles, reduce=1., smooth=False, ksize=3, sigma=1., check=True, info=None):
    """Make a mesh (in MODEL coordinates) the frozen template of `model`: signed_distance_grid over the model's own box and
    world_size, then model.init_sdf_from_sdf(sdf, smooth, reduce, ksize, sigma).
        vertices, triangles = mesh.read_ply('probe.ply')
        mesh.voxurf_template_from_mesh(model, vertices, triangles)
    -> the [X,Y,Z] grid signed_distance_grid returned (with the defaults model.sdf.grid holds its bits)."""
    dev = model.sdf.grid.device
    v = torch.from_numpy(np.array(vertices, dtype=np.float32)).to(dev) if isinstance(vertices, np.ndarray) else vertices
    sdf = signed_distance_grid(v, triangles, model.xyz_min, model.xyz_max, [int(s) for s in model.world_size.tolist()],
                               check=check, info=info)
    model.init_sdf_from_sdf(sdf[None, None], smooth=smooth, reduce=reduce, ksize=ksize, sigma=sigma)
    return sdf
