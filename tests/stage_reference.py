"""Plain-autograd references of the object-branch stage kernels, parameterised by dtype (CPU, torch).

Each function restates the forward of one stage from the reference model's expressions and differentiates it with
torch.autograd; none of them restates the hand derivation the kernels implement (that is tests/analytic_model.py, which is
deliberately not used here).  Run in float64 they are the yardstick of tests/test_hip_stage_kernels.py; run in float32 they
give the error a straightforward fp32 evaluation of the same maths makes, and tests/test_stage_reference.py pins them to the
reference's own outputs.

Layouts follow the kernels: the SDF template is [X,Y,Z], the colour grid is given in the reference's [C,X,Y,Z] layout (the
kernels read it channels-last), warp outputs are [M,16] = [deform(3), correction, then for i = 0..2: d q_j / d p_i (j = 0..2)
minus delta_ij, d correction / d p_i].
"""
import torch
import torch.nn.functional as F

from oracle import native_ops
from oracle import voxurf_oracle as O

FEAT_LD = 64


def _t(x, dtype):
    return torch.as_tensor(x).detach().to(dtype).clone()


def _leaf(x, dtype):
    return _t(x, dtype).requires_grad_(True)


def grid_u(p, mn, mx, size):
    """World coordinate -> voxel coordinate, in the reference's order of operations (normalise to [-1,1], then
    grid_sample's align_corners unnormalisation)."""
    n = (p - mn) / (mx - mn) * 2 - 1
    return ((n + 1) / 2) * (size - 1)


def sdf_lookup(grid, q, mn, mx, A, B):
    """grid_sample_3d (use_custom) of the mapped template A * (sigmoid(B * sdf) - 0.5) at q [M,3]: weights from the unclamped
    floor, clamped corner indices.  A, B: [M] (per-sample copies of the two mapped scalars)."""
    size = grid.shape
    u = [grid_u(q[:, a], mn[a], mx[a], size[a]) for a in range(3)]
    with torch.no_grad():
        f = [torch.floor(x) for x in u]
    out = 0
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = 1
                idx = []
                for a, d in enumerate((dx, dy, dz)):
                    w = w * ((u[a] - f[a]) if d else (f[a] + 1 - u[a]))
                    idx.append(torch.clamp(f[a] + d, 0, size[a] - 1).long())
                S = grid[idx[0], idx[1], idx[2]]
                out = out + A * (torch.sigmoid(B * S) - 0.5) * w
    return out


def _dot(g, x, dtype):
    return (_t(g, dtype) * x).sum() if g is not None else 0


def geometry(p, wo, viewdirs, ray_id, sdf_grid, sdf_ab, inv_s, dist, xyz_min, xyz_max, dtype=torch.float64,
             g_alpha=None, g_gradient=None, g_sdf_final=None, g_sdf_deform=None, g_grad_deform=None, g_correction=None,
             priors=None):
    """pp_geometry_fwd / pp_geometry_bwd(_priors) for M samples.

    Forward: q = p + deform, sdf = tri(q) + correction, gradient = A grad_q tri + J_c with A = I + wo[4 + 4i + j], NeuS alpha
    (use_mid, cos_anneal_ratio 1) clipped to [0, 1].  Backward: autograd of the inner product of the upstream gradients with the
    outputs (None = zero) plus, with priors = (w_eik, w_dyn, loss_scale, n_norm), the sample terms of object_losses.
    Returns a dict of outputs and gradients; `vgrad_s` is the per-sample viewdir gradient, `sdf_ab_rows` the per-sample
    contribution to the sdf_ab gradient (its sum is `sdf_ab`)."""
    M = p.shape[0]
    p, wo = _leaf(p, dtype), _leaf(wo, dtype)
    vs = _leaf(torch.as_tensor(viewdirs)[torch.as_tensor(ray_id).long()], dtype)
    ab = _leaf(torch.as_tensor(sdf_ab).reshape(1, 2).repeat(M, 1), dtype)
    grid = _t(sdf_grid, dtype)
    mn, mx = _t(xyz_min, dtype), _t(xyz_max, dtype)
    A = F.softplus(ab[:, 0], beta=10)
    B = F.softplus(ab[:, 1], beta=10)
    q = p + wo[:, :3]
    vq = sdf_lookup(grid, q, mn, mx, A, B)
    gq = torch.autograd.grad(vq.sum(), q, create_graph=True)[0]
    W = wo.view(M, 4, 4)
    Amat = torch.eye(3, dtype=dtype) + W[:, 1:, :3]
    gradient = (Amat * gq[:, None, :]).sum(-1) + W[:, 1:, 3]
    corr = wo[:, 3]
    sdf = vq + corr
    sdf_deform = sdf - sdf_lookup(grid, p, mn, mx, A, B)
    cos = (vs * gradient).sum(-1)
    ic = -F.relu(-cos)
    nxt = sdf + ic * dist * 0.5
    prv = sdf - ic * dist * 0.5
    pc, nc = torch.sigmoid(prv * inv_s), torch.sigmoid(nxt * inv_s)
    a_un = ((pc - nc) + 1e-5) / (pc + 1e-5)
    alpha = a_un.clip(0.0, 1.0)
    L = (_dot(g_alpha, alpha, dtype) + _dot(g_gradient, gradient, dtype) + _dot(g_sdf_final, sdf, dtype)
         + _dot(g_sdf_deform, sdf_deform, dtype) + _dot(g_grad_deform, Amat.reshape(M, 9), dtype)
         + _dot(g_correction, corr, dtype))
    losses = None
    if priors is not None:
        w_eik, w_dyn, ls, n = priors
        eik = torch.abs(gradient.norm(dim=-1) - 1).sum() / n
        gd = Amat.norm(dim=-1).sum() / (3 * n)
        c = torch.abs(corr).sum() / n
        sd = torch.abs(sdf_deform).sum() / n
        L = L + ls * (w_eik * eik + w_dyn * (gd + c + sd))
        losses = torch.stack([eik, gd, c, sd]).detach()
    out = {'alpha': alpha.detach(), 'gradient': gradient.detach(), 'sdf_final': sdf.detach(),
           'sdf_deform': sdf_deform.detach(), 'grad_deform': Amat.detach().reshape(M, 9), 'a_un': a_un.detach(),
           'cos': cos.detach(), 'losses': losses, 'pc': pc.detach(), 'nc': nc.detach(), 'gq': gq.detach(), 'A': A.detach()}
    if isinstance(L, torch.Tensor) and L.requires_grad:
        gwo, gp, gv, gab = torch.autograd.grad(L, [wo, p, vs, ab], allow_unused=True)
        z = lambda g, x: torch.zeros_like(x) if g is None else g
        out.update(warp_out_grad=z(gwo, wo), pts_grad=z(gp, p), vgrad_s=z(gv, vs), sdf_ab_rows=z(gab, ab))
        out['sdf_ab'] = out['sdf_ab_rows'].sum(0)
    return out


def color_feat(k0, pts, viewdirs, ray_id, gradient, pe_w, Lp, Lv, xyz_min, xyz_max, dtype=torch.float64, feat_grad=None):
    """pp_color_feat_fwd / _bwd: [k0 lookup (zeros padding) | t, w_k sin(2^k t), w_k cos(2^k t) | v, ... | normal] padded with
    zeros to 64 columns; pe_w = [position weights (Lp) | view weights (Lv)].  k0 is [C,X,Y,Z].  Backward (feat_grad [M,64]):
    k0 (dense, [C,X,Y,Z]), pts, gradient and the per-sample viewdir."""
    M = pts.shape[0]
    k0 = _leaf(k0, dtype)
    p, g = _leaf(pts, dtype), _leaf(gradient, dtype)
    vs = _leaf(torch.as_tensor(viewdirs)[torch.as_tensor(ray_id).long()], dtype)
    mn, mx = _t(xyz_min, dtype), _t(xyz_max, dtype)
    pw = _t(pe_w, dtype)
    coords = ((p - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    kf = F.grid_sample(k0[None], coords.reshape(1, 1, 1, M, 3), mode='bilinear', align_corners=True, padding_mode='zeros')
    kf = kf.reshape(k0.shape[0], M).T

    def enc(x, L, w):
        freq = torch.tensor([2. ** i for i in range(L)], dtype=dtype)
        emb = (x.unsqueeze(-1) * freq).flatten(-2)
        return torch.cat([x, emb.sin() * w.repeat(3), emb.cos() * w.repeat(3)], -1)

    t = (p - mn) / (mx - mn)
    normal = g / (g.norm(dim=-1, keepdim=True) + 1e-5)
    feat = torch.cat([kf, enc(t, Lp, pw[:Lp]), enc(vs, Lv, pw[Lp:Lp + Lv]), normal], -1)
    feat = F.pad(feat, (0, FEAT_LD - feat.shape[1]))
    out = {'feat': feat.detach()}
    if feat_grad is not None:
        gk, gp, gg, gv = torch.autograd.grad((feat * _t(feat_grad, dtype)).sum(), [k0, p, g, vs], allow_unused=True)
        out.update(k0_grad=gk, pts_grad=gp, gradient_grad=gg, vgrad_s=gv)
    return out


def _segments(ray_start):
    rs = torch.as_tensor(ray_start).long()
    N = rs.numel() - 1
    ray_id = torch.repeat_interleave(torch.arange(N), rs[1:] - rs[:-1])
    return rs, N, ray_id


def march(alpha, rgb, ray_start, bg, step_w=None, nrm=None, dtype=torch.float64, clamp=True, g_rgbm=None, g_cw=None,
          g_last=None, g_depth=None, g_w=None):
    """pp_march_fwd / _bwd.  The transmittance scan (weights, T, alphainv_last, i_end) is the reference's bit-exact float/double
    recurrence with the 1e-3 stop (oracle.native_ops); everything after it is `dtype` autograd, with each weight the function
    alpha_i * prod_{j<i} (1 - alpha_j) of the alphas for i < i_end (0 past it) and alphainv_last = prod_{j<i_end} (1 - alpha_j).
    clamp=False: rgb_marched is the unclamped sum (the backward's behaviour when no rgb_pre is given)."""
    rs, N, ray_id = _segments(ray_start)
    a32 = torch.as_tensor(alpha).float()
    w32, T32, last32, _, i_end = native_ops.alpha2weight(a32, ray_id, N)
    a = _leaf(a32, dtype)
    r = _leaf(rgb, dtype)
    live = torch.zeros(a.numel(), dtype=torch.bool)
    ws, lasts = [], []
    for k in range(N):
        b, e = int(rs[k]), int(rs[k + 1])
        if e == b:
            ws.append(a[b:e])
            lasts.append(torch.ones((), dtype=dtype))
            continue
        ie = int(i_end[k])
        live[b:ie] = True
        om = 1 - a[b:ie]
        Tk = torch.cat([torch.ones(1, dtype=dtype), torch.cumprod(om, 0)])
        ws.append(torch.cat([a[b:ie] * Tk[:-1], torch.zeros(e - ie, dtype=dtype)]))
        lasts.append(Tk[-1])
    w = torch.cat(ws)
    last = torch.stack(lasts)
    seg = lambda x: torch.zeros((N,) + x.shape[1:], dtype=dtype).index_add(0, ray_id, x)
    cw = seg(w)
    pre = seg(w[:, None] * r) + (1 - cw)[:, None] * bg
    rgbm = pre.clamp(0, 1) if clamp else pre
    out = {'weights32': w32, 'T32': T32, 'last32': last32, 'i_end': i_end, 'weights': w.detach(), 'alphainv_last': last.detach(),
           'cum_weights': cw.detach(), 'rgb_pre': pre.detach(), 'rgb_marched': rgbm.detach()}
    L = _dot(g_rgbm, rgbm, dtype) + _dot(g_cw, cw, dtype) + _dot(g_last, last, dtype) + _dot(g_w, w, dtype)
    if step_w is not None:
        depth = seg(w * _t(step_w, dtype))
        out['depth_acc'] = depth.detach()
        L = L + _dot(g_depth, depth, dtype)
    if nrm is not None:
        out['normal_marched'] = seg(w[:, None] * _t(nrm, dtype)).detach()
    if isinstance(L, torch.Tensor) and L.requires_grad:
        ga, gr = torch.autograd.grad(L, [a, r], allow_unused=True)
        out['g_alpha'] = torch.zeros_like(a) if ga is None else ga
        out['g_rgb'] = torch.zeros_like(r) if gr is None else gr
    return out


def march_dvgo(alpha, rgb, step_w, ray_start, dtype=torch.float64):
    """pp_march_dvgo_fwd: weights = alpha * exclusive cumprod of clamp_min(1 - alpha, 1e-10), no early stop (dvgo_ori.py)."""
    rs, N, ray_id = _segments(ray_start)
    a = _t(alpha, dtype)
    T = torch.empty_like(a)
    last = torch.ones(N, dtype=dtype)
    for k in range(N):
        b, e = int(rs[k]), int(rs[k + 1])
        if e > b:
            c = O.cumprod_exclusive((1 - a[b:e])[None])[0]
            T[b:e], last[k] = c[:-1], c[-1]
    w = a * T
    seg = lambda x: torch.zeros((N,) + x.shape[1:], dtype=dtype).index_add(0, ray_id, x)
    return {'weights': w, 'T': T, 'alphainv_last': last, 'cum_weights': seg(w), 'rgb_acc': seg(w[:, None] * _t(rgb, dtype)),
            'depth_acc': seg(w * _t(step_w, dtype))}


def slab_t_min(rays_o, rays_d, xyz_min, xyz_max, near, far):
    """t_min of sample_ray_ori (voxurf_coarse.py:697-705), differentiable like the reference."""
    vec = torch.where(rays_d == 0, torch.full_like(rays_d, 1e-6), rays_d)
    rate_a = (xyz_max - rays_o) / vec
    rate_b = (xyz_min - rays_o) / vec
    return torch.minimum(rate_a, rate_b).amax(-1).clamp(min=near, max=far)


def raygen_select_bwd(c2w, Ks, H, W, ray_idx, ray_start, pts_grad, step, xyz_min, xyz_max, near, far, vgrad_s=None,
                      g_depth=None, dtype=torch.float64):
    """pp_raygen_select_bwd: rays from c2w (Voxurf variant, rays_d = viewdirs = normalised), samples
    p = o + d (t_min + step / |d|), depth = t_min / |d| (+ terms independent of the rays).  Autograd of
    <pts_grad, p> + <vgrad_s, viewdir of the sample's ray> + <g_depth, depth> with respect to c2w and, for the call form
    without cameras, with respect to rays_o / rays_d / viewdirs as three separate leaves."""
    rs, N, ray_id = _segments(ray_start)
    c2w = _leaf(c2w, dtype)
    Ks = _t(Ks, dtype)
    idx = torch.as_tensor(ray_idx).long()
    view = idx // (H * W)
    rem = idx - view * (H * W)
    pj, pi = rem // W, rem - (rem // W) * W
    o = torch.zeros(N, 3, dtype=dtype)
    d = torch.zeros(N, 3, dtype=dtype)
    for v in range(c2w.shape[0]):
        sel = (view == v).nonzero()[:, 0]
        if len(sel):
            ov, dv, _ = O.rays_at_pixels(pi[sel].to(dtype), pj[sel].to(dtype), Ks[v], c2w[v])
            o, d = o.index_put((sel,), ov), d.index_put((sel,), dv)

    def loss(o, d, vd):
        mn, mx = _t(xyz_min, dtype), _t(xyz_max, dtype)
        tm = slab_t_min(o, d, mn, mx, near, far)
        nrm = d.norm(dim=-1)
        pts = o[ray_id] + d[ray_id] * (tm[ray_id] + _t(step, dtype) / nrm[ray_id])[:, None]
        L = (pts * _t(pts_grad, dtype)).sum()
        if vgrad_s is not None:
            L = L + (vd[ray_id] * _t(vgrad_s, dtype)).sum()
        if g_depth is not None:
            L = L + (_t(g_depth, dtype) * tm / nrm).sum()
        return L

    gc = torch.autograd.grad(loss(o, d, d), [c2w])[0]
    ol, dl, vl = _leaf(o, dtype), _leaf(d, dtype), _leaf(d, dtype)
    go, gd, gv = torch.autograd.grad(loss(ol, dl, vl), [ol, dl, vl], allow_unused=True)
    return {'c2w_grad': gc, 'g_o': go, 'g_d': gd, 'g_v': torch.zeros_like(vl) if gv is None else gv,
            'rays_o': o.detach(), 'rays_d': d.detach()}


def grid_sample(grid, pts, xyz_min, xyz_max, border, dtype=torch.float64, out_grad=None):
    """pp_grid_sample_fwd / _bwd: F.grid_sample (bilinear, align_corners, zeros or border padding) of grid [C,X,Y,Z] at
    world points with the reference's x<->z flip; backward with respect to the grid and the points."""
    M = pts.shape[0]
    g, p = _leaf(grid, dtype), _leaf(pts, dtype)
    mn, mx = _t(xyz_min, dtype), _t(xyz_max, dtype)
    coords = ((p - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    out = F.grid_sample(g[None], coords.reshape(1, 1, 1, M, 3), mode='bilinear', align_corners=True,
                        padding_mode='border' if border else 'zeros').reshape(g.shape[0], M).T
    res = {'out': out.detach()}
    if out_grad is not None:
        gg, gp = torch.autograd.grad((out * _t(out_grad, dtype)).sum(), [g, p])
        res.update(grid_grad=gg, pts_grad=gp)
    return res


def first_crossing(sdf_dense, t_min, rays_o, rays_d, dist, dtype=torch.float64):
    """pp_sdf_first_crossing against oracle.query_first_crossing on a dense [N,S] row."""
    class _S:
        stepsize, voxel_size = dist, 1.0
    sd = _t(sdf_dense, dtype)
    pts, hit = O.query_first_crossing(_S, sd, _t(t_min, dtype), _t(rays_o, dtype), _t(rays_d, dtype))
    return pts, hit
