"""Float64 restatement of the surface-projection feature loss (lib/recon_scene.py:371-439), from the two queries' rays, entry
distances and expected depths on - steps 2 to 7 of the term, everything but the renderer:

  :389-396, lib/common.py:450-465    `reproject`: p into view j, near-plane replacement, pixel
  :410-411                           |p - p_ref| < 2 voxel_size, both hit flags
  :413-419, lib/camera.py:251-253    world2cam into views i and j with the near-plane replacement (a constant: no gradient)
  :427-429, lib/common.py:468-492    normalised coordinates, max(|x|, |y|) <= 1 in both views
  :430-438, lib/common.py:76-109     grid_sample (bilinear, align_corners, zero padding), cosine similarity, 1 - mean over valid rows
plus the generators that rebuild a case's feature maps from its name (they are never stored) and the parameters of the recorded
case.  The gradients come from torch autograd over the formula, in whatever dtype the caller asks for."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# the recorded case (tools/make_featproj_golden.py): G = 24, three 32 x 32 views, global_step 50, 96 rows, two layers
G, H, W, NV, GS, ROWS = 24, 32, 32, 3, 50, 96
LAYERS = ((256, 8, 8), (20, 11, 7))                 # (C, h, w)
PARAM_SEED = 23                                     # the `g24` parameter set of oracle/make_golden.py (gen_query / gen_reproj)
RENDER_KWARGS = dict(near=0.24, far=4.8, bg=0, stepsize=1.5, inverse_y=True, flip_x=False, flip_y=False)
MARGIN = 1e-3                                       # no row of a recorded case lies within this (relative) of a decision


def feature_maps(case, n_views, layers, noise=0.05):
    """Per layer (C, h, w) a map [n_views, C, h, w] float32: a smooth random field (a 4 x 4 lattice of normal draws, interpolated
    linearly) plus `noise` x white noise, from numpy's RandomState seeded by the case name - the same bits wherever it runs."""
    out = []
    for li, (C, h, w) in enumerate(layers):
        rng = np.random.RandomState(zlib.crc32(f'{case}/{li}'.encode()) & 0x7FFFFFFF)
        lat = rng.randn(n_views, C, 4, 4)
        ys, xs = np.linspace(0, 3, h), np.linspace(0, 3, w)
        y0, x0 = np.minimum(ys.astype(int), 2), np.minimum(xs.astype(int), 2)
        ty, tx = (ys - y0)[:, None], (xs - x0)[None, :]
        rows = lat[:, :, y0] * (1 - ty)[None, None] + lat[:, :, y0 + 1] * ty[None, None]                  # [V,C,h,4]
        field = rows[:, :, :, x0] * (1 - tx)[None, None] + rows[:, :, :, x0 + 1] * tx[None, None]           # [V,C,h,w]
        out.append(torch.tensor((field + noise * rng.randn(n_views, C, h, w)).astype(np.float32)))
    return out


def fixture_params():
    """The recorded case's parameters, regenerated from the seed (the set reproj_g24.npz stores)."""
    from oracle import voxurf_oracle as O
    from tests.helpers import scene_for
    return O.init_params(scene_for(G), seed=PARAM_SEED)


def param_checksum(P):
    flat = [P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta']] + [t for net in ('rgbnet', 'warp') for Wb in P[net] for t in Wb]
    return np.array([float(t.double().abs().sum()) for t in flat])


def intr_of(Ks):
    Ks = np.asarray(Ks)
    return np.stack([Ks[:, 0, 0], Ks[:, 1, 1], Ks[:, 0, 2], Ks[:, 1, 2]], -1)


def _cam(w2c, v, p, nl):
    q = p @ w2c[v, :, :3].T + w2c[v, :, 3]
    behind = q[:, 2] < nl
    return torch.where(behind[:, None], torch.full_like(q, nl), q), behind


def _pixel(intr, v, q):
    fx, fy, cx, cy = intr[v]
    return torch.stack([(fx * q[:, 0] + cx * q[:, 2]) / q[:, 2], (fy * q[:, 1] + cy * q[:, 2]) / q[:, 2]], -1)


def reproject(o, d, t_min, acc, w2c, intr, j, nl, dtype=torch.float64):
    """Step 2: the pixel of view j that query B shoots through, per row [R,2]."""
    c = lambda t: torch.as_tensor(t).to(dtype)
    o, d, t_min, acc, w2c, intr = (c(t) for t in (o, d, t_min, acc, w2c, intr))
    p = o + d * (t_min + acc)[:, None]
    q, _ = _cam(w2c, j, p, nl)
    return _pixel(intr, j, q)


def decisions(qa, qb, w2c, intr, i, j, nl, voxel, H, W, dtype=torch.float64):
    """The quantities the flags compare, per row: dict(gap = |p - p_ref|, limit = 2 voxel, xy [R,4] = (x_i, y_i, x_j, y_j),
    qz [R,2] = raw q_z in views i and j, acc [R,2]) and, per cause, which rows it rejects."""
    c = lambda t: torch.as_tensor(t).to(dtype)
    w2c, intr = c(w2c), c(intr)
    pa = c(qa['o']) + c(qa['d']) * (c(qa['t_min']) + c(qa['acc']))[:, None]
    pb = c(qb['o']) + c(qb['d']) * (c(qb['t_min']) + c(qb['acc']))[:, None]
    gap = (pa - pb).norm(dim=-1)
    xy, qz = [], []
    for v in (i, j):
        qz.append((pa @ w2c[v, :, :3].T + w2c[v, :, 3])[:, 2])
        q, _ = _cam(w2c, v, pa, nl)
        u = _pixel(intr, v, q)
        xy += [2 * u[:, 0] / (W - 1) - 1, 2 * u[:, 1] / (H - 1) - 1]
    xy, qz = torch.stack(xy, -1), torch.stack(qz, -1)
    acc = torch.stack([c(qa['acc']), c(qb['acc'])], -1)
    reject = dict(far=~(gap < 2 * voxel), miss=~(acc[:, 0] > 0), miss_ref=~(acc[:, 1] > 0),
                  outside_i=~(xy[:, :2].abs().amax(-1) <= 1), outside_j=~(xy[:, 2:].abs().amax(-1) <= 1))
    return dict(gap=gap, limit=2 * voxel, xy=xy, qz=qz, acc=acc, reject=reject)


def row_margins(dec, nl):
    """Per row, the smallest relative distance to any decision: |gap - limit| / limit, ||x| - 1|, |q_z - nl| / nl, and acc itself
    (a depth in scene units of order 1).  acc is exactly 0 for a ray without a sample: no near-tie.  A ray that crosses the box
    beside the surface has acc ~ 1e-8, the rounding noise of the NeuS alpha's difference of sigmoids: a tie."""
    acc = torch.where(dec['acc'] == 0, torch.full_like(dec['acc'], float('inf')), dec['acc'].abs())
    parts = [((dec['gap'] - dec['limit']).abs() / dec['limit'])[:, None], (dec['xy'].abs() - 1).abs(), (dec['qz'] - nl).abs() / nl, acc]
    return torch.cat(parts, -1).amin(-1)


def decision_margin(dec, nl):
    return float(row_margins(dec, nl).min())


def restate(qa, qb, w2c, intr, i, j, nl, voxel, H, W, feats, weight=1.0, scale=1.0, dtype=torch.float64, n_rows=None):
    """Steps 3 to 7.  qa / qb: dict(o [R,3], d [R,3], t_min [R], acc [R]) of query A / B; feats: list of [V,C,h,w]; intr [V,4]
    (fx, fy, cx, cy).  Rows from n_rows on are none.  -> dict(loss, n_valid, valid [R] bool, cos [L,R] (0 where not valid),
    sum_cos [L], g_o, g_d [R,3], g_depth [R], g_w2c [V,3,4]: the gradient of scale * weight * loss on query A's ray origin,
    direction and depth (p = o + d depth) and on w2c).  Without a valid row: loss 0 and zero gradients (the reference: NaN)."""
    c = lambda t: torch.as_tensor(t).detach().to(dtype).clone()
    o, d = c(qa['o']).requires_grad_(True), c(qa['d']).requires_grad_(True)
    depth = (c(qa['t_min']) + c(qa['acc'])).requires_grad_(True)
    Wm = c(w2c).requires_grad_(True)
    K = c(intr)
    R = o.shape[0]
    n_rows = R if n_rows is None else n_rows
    p = o + d * depth[:, None]
    with torch.no_grad():
        p_ref = c(qb['o']) + c(qb['d']) * (c(qb['t_min']) + c(qb['acc']))[:, None]
        close = (p - p_ref).norm(dim=-1) < 2 * voxel                                                   # :410
        ok = close & (c(qb['acc']) > 0) & (c(qa['acc']) > 0) & (torch.arange(R) < n_rows)                # :411
    xy = []
    for v in (i, j):
        q, _ = _cam(Wm, v, p, nl)                                                                         # :413-419
        u = _pixel(K, v, q)
        xy.append(torch.stack([2 * u[:, 0] / (W - 1) - 1, 2 * u[:, 1] / (H - 1) - 1], -1))              # common.py:485-486
    valid = ok & (xy[0].detach().abs().amax(-1) <= 1) & (xy[1].detach().abs().amax(-1) <= 1)             # common.py:488, :428-429
    n_valid = int(valid.sum())
    L = len(feats)
    cos = torch.zeros(L, R, dtype=dtype)
    z = torch.zeros
    if n_valid == 0:
        return dict(loss=z((), dtype=dtype), n_valid=0, valid=valid, cos=cos, sum_cos=z(L, dtype=dtype), g_o=z(R, 3, dtype=dtype),
                    g_d=z(R, 3, dtype=dtype), g_depth=z(R, dtype=dtype), g_w2c=z(*Wm.shape, dtype=dtype))
    grid = torch.stack(xy)[:, None]                                                                       # [2,1,R,2]
    loss = 0.
    for l, feat in enumerate(feats):
        val = F.grid_sample(c(feat)[[i, j]], grid, mode='bilinear', padding_mode='zeros', align_corners=True)[:, :, 0].permute(0, 2, 1)
        cs = F.cosine_similarity(val[0][valid], val[1][valid], dim=-1)                                   # :435-437
        cos[l, valid] = cs.detach()
        loss = loss + (1 - cs.mean())
    (scale * weight * loss).backward()
    return dict(loss=loss.detach(), n_valid=n_valid, valid=valid, cos=cos, sum_cos=cos.sum(1), g_o=o.grad, g_d=d.grad,
                g_depth=depth.grad, g_w2c=Wm.grad)
