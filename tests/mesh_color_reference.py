"""Plain-torch restatement of the vertex attributes of poseprobe_amd.mesh.vertex_attributes, runnable in
float32 and float64 on the CPU: the arithmetic of the render path's colour stage with the ray removed.

    params(source)                      the model's tensors as a dict of CPU tensors (a Voxurf, or a golden fixture's arrays)
    vertex_attributes(P, pts, ...)      dict(normals, colors, gradient, feat, q_u) in `dtype`
    face_mask(q_u, tol)                 vertices whose warped point lies within `tol` voxels of a cell face (the gradient of the
                                        deformed sdf is discontinuous there)

Per vertex p (model coordinates):
    use_deform=True    (d, c) = warp(p) * output_range, q = p + d, sdf = mapped template(q) + c, g = d sdf / d p by autograd
    use_deform=False   g = the trilinear lookup (border padding) of the central differences of the mapped template
    normal = g / (|g| + 1e-5), viewdir = -normal
    feat = [k0(p) (zero padding) | PE_pos(p) | PE_view(viewdir) | normal], BARF weights from `progress`
    rgb = sigmoid(rgbnet(feat))
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def params(source, barf_c2f=(0.6, 1.0), N_iters=10000):
    """source: a Voxurf (its state dict is read; barf_c2f / N_iters come from the module), or the arrays of a golden fixture
    (`P.*` keys, the synthetic box of poseprobe_amd.synthetic)."""
    if hasattr(source, 'state_dict'):
        sd = {k: v.detach().cpu() for k, v in source.state_dict().items()}
        warp_key = 'warp_network.deform_net.net.net.{}.0.{}'
        rg_keys = ['rgbnet.0', 'rgbnet.2.0', 'rgbnet.3.0', 'rgbnet.4']
        return dict(xyz_min=sd['xyz_min'].float(), xyz_max=sd['xyz_max'].float(), sdf=sd['sdf.grid'][0, 0].float(),
                    k0=sd['k0.grid'][0].float().contiguous(), sdf_alpha=sd['sdf_alpha'].float(), sdf_beta=sd['sdf_beta'].float(),
                    rgbnet=[(sd[k + '.weight'].float(), sd[k + '.bias'].float()) for k in rg_keys],
                    warp=[(sd[warp_key.format(i, 'weight')].float(), sd[warp_key.format(i, 'bias')].float()) for i in range(5)],
                    out_range=float(source.warp_network.output_range), voxel_size=float(source.voxel_size),
                    barf_c2f=None if source.barf_c2f is None else tuple(source.barf_c2f), N_iters=int(source.N_iters),
                    progress=float(sd['progress']))
    from poseprobe_amd import synthetic as syn
    d = source
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)
    lo, hi = t(syn.XYZ_MIN), t(syn.XYZ_MAX)
    G = int(d['G'])
    return dict(xyz_min=lo, xyz_max=hi, sdf=t(d['P.sdf'])[0, 0], k0=t(d['P.k0'])[0], sdf_alpha=t(d['P.sdf_alpha']),
                sdf_beta=t(d['P.sdf_beta']), rgbnet=[(t(d[f'P.rgbnet.{i}.weight']), t(d[f'P.rgbnet.{i}.bias'])) for i in range(4)],
                warp=[(t(d[f'P.warp.{i}.weight']), t(d[f'P.warp.{i}.bias'])) for i in range(5)],
                out_range=float(syn.range_shape().max()), voxel_size=float(((hi - lo).prod() / G ** 3).pow(1 / 3)),
                barf_c2f=barf_c2f, N_iters=N_iters, progress=0.0)


def mlp(layers, x, dtype):
    for i, (W, b) in enumerate(layers):
        x = F.linear(x, W.to(dtype), b.to(dtype))
        if i < len(layers) - 1:
            x = F.relu(x)
    return x


def mapped_template(P, dtype):
    sp = lambda t: F.softplus(t.to(dtype), beta=10)
    return sp(P['sdf_alpha']) * (torch.sigmoid(sp(P['sdf_beta']) * P['sdf'].to(dtype)) - 0.5)


def grid_u(P, p, size, dtype):
    """world -> continuous voxel coordinate, the order of operations of the samplers: ((t 2 - 1) + 1) / 2 (size - 1)."""
    lo, hi = P['xyz_min'].to(dtype), P['xyz_max'].to(dtype)
    t = (p - lo) / (hi - lo)
    return ((t * 2 - 1) + 1) / 2 * (torch.tensor(size, dtype=dtype) - 1)


def _corners(u, size, pad):
    """-> per corner c = dx 4 + dy 2 + dz: (flat index [n], weight [n], inside [n]).  pad: 'custom' (weights from the unclamped floor,
    indices clamped: the reference's own sdf sampler), 'border' (coordinate clamped first), 'zeros' (outside corners weigh nothing)."""
    X, Y, Z = size
    top = torch.tensor([X - 1, Y - 1, Z - 1], dtype=u.dtype)
    if pad == 'border':
        u = torch.minimum(torch.maximum(u, torch.zeros_like(u)), top.expand_as(u))
    f = torch.floor(u).detach()
    w1, w0 = u - f, (f + 1) - u
    i0 = f.long()
    out = []
    for c in range(8):
        d = torch.tensor([(c >> 2) & 1, (c >> 1) & 1, c & 1])
        i = i0 + d
        inside = ((i >= 0) & (i <= top.long())).all(-1)
        ic = torch.minimum(torch.maximum(i, torch.zeros_like(i)), top.long().expand_as(i))
        w = torch.where(d.bool(), w1, w0).prod(-1)
        out.append(((ic[:, 0] * Y + ic[:, 1]) * Z + ic[:, 2], w, inside))
    return out


def sample(grid, u, pad):
    """grid [X,Y,Z] or [C,X,Y,Z] at voxel coordinates u [n,3] -> [n] or [n,C]."""
    size = tuple(grid.shape[-3:])
    flat = grid.reshape(-1, size[0] * size[1] * size[2]) if grid.dim() == 4 else grid.reshape(1, -1)
    acc = 0
    for idx, w, inside in _corners(u, size, pad):
        if pad == 'zeros':
            w = w * inside.to(w.dtype)
        acc = acc + flat[:, idx] * w
    return acc[0] if grid.dim() == 3 else acc.t()


def central_differences(G, voxel_size):
    """neus_sdf_gradient, grad_mode='interpolate': (G[n + 1] - G[n - 1]) / 2 / voxel_size, zero on the two boundary planes."""
    D = torch.zeros(3, *G.shape, dtype=G.dtype)
    D[0, 1:-1] = (G[2:] - G[:-2]) / 2 / voxel_size
    D[1, :, 1:-1] = (G[:, 2:] - G[:, :-2]) / 2 / voxel_size
    D[2, :, :, 1:-1] = (G[:, :, 2:] - G[:, :, :-2]) / 2 / voxel_size
    return D


def pe_weights(P, progress, L, dtype):
    if P['barf_c2f'] is None:
        return torch.ones(L, dtype=dtype)
    start, end = P['barf_c2f']
    alpha = (torch.tensor(progress, dtype=dtype) - start) / (end - start) * L
    return (1 - ((alpha - torch.arange(L, dtype=dtype)).clamp(0, 1) * math.pi).cos()) / 2


def encode(x, w):
    """[x | w_k sin(2^k x_a) (a major, k minor) | w_k cos(...)]"""
    L = w.shape[0]
    ang = x[:, :, None] * (2.0 ** torch.arange(L, dtype=x.dtype))
    return torch.cat([x, (ang.sin() * w).reshape(len(x), -1), (ang.cos() * w).reshape(len(x), -1)], -1)


def deform_sdf(P, pts, dtype):
    """-> (sdf [n], voxel coordinate of the warped point [n,3]); differentiable in pts."""
    out = mlp(P['warp'], pts, dtype) * P['out_range']
    q_u = grid_u(P, pts + out[:, :3], P['sdf'].shape, dtype)
    return sample(mapped_template(P, dtype), q_u, 'custom') + out[:, 3], q_u


def vertex_attributes(P, pts, use_deform=True, progress=None, dtype=torch.float64, Lp=5, Lv=1):
    pts = (pts.detach().cpu() if isinstance(pts, torch.Tensor) else torch.tensor(np.array(pts))).to(dtype)
    progress = P['progress'] if progress is None else progress
    lo, hi = P['xyz_min'].to(dtype), P['xyz_max'].to(dtype)
    q_u = None
    if use_deform:
        p = pts.clone().requires_grad_(True)
        sdf, q_u = deform_sdf(P, p, dtype)
        g, = torch.autograd.grad(sdf.sum(), p)
        q_u = q_u.detach()
    else:
        with torch.no_grad():
            D = central_differences(mapped_template(P, dtype), torch.tensor(P['voxel_size'], dtype=dtype))
            g = sample(D, grid_u(P, pts, P['sdf'].shape, dtype), 'border')
    with torch.no_grad():
        normal = g / (g.norm(dim=-1, keepdim=True) + 1e-5)
        k0 = sample(P['k0'].to(dtype), grid_u(P, pts, P['k0'].shape[-3:], dtype), 'zeros')
        feat = torch.cat([k0, encode((pts - lo) / (hi - lo), pe_weights(P, progress, Lp, dtype)),
                          encode(-normal, pe_weights(P, progress, Lv, dtype)), normal], -1)
        colors = torch.sigmoid(mlp(P['rgbnet'], feat, dtype))
    return dict(normals=normal, colors=colors, gradient=g.detach(), feat=feat, q_u=q_u)


def face_mask(q_u, tol=1e-3):
    """True where a coordinate of q (in voxels) lies within tol of an integer: a cell face of the template."""
    return ((q_u - torch.round(q_u)).abs() < tol).any(-1)


def deform_vertices(P, resolution, dtype=torch.float64):
    """Vertices of the deformed zero level set on the model's box at a lattice resolution, with the numpy marching cubes of
    tests/mesh_reference.py: what mesh.voxurf_extract_deform_geometry extracts, restated (model coordinates, float32)."""
    from tests import mesh_reference as R
    lo, hi = P['xyz_min'], P['xyz_max']
    axes = [torch.linspace(float(lo[a]), float(hi[a]), resolution) for a in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing='ij'), dim=-1).reshape(-1, 3)
    with torch.no_grad():
        u = -deform_sdf(P, pts.to(dtype), dtype)[0]
    v, _ = R.marching_cubes(u.reshape(resolution, resolution, resolution).float().numpy(), 0.0)
    return (v / (resolution - 1.0) * (hi - lo).numpy()[None] + lo.numpy()[None]).astype(np.float32)
