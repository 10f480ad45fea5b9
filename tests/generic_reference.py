"""Plain-autograd references of the kernels behind the DirectVoxGO twin (poseprobe_amd/dvgo_ori.py), parameterised by dtype
(CPU, torch), in the style of tests/stage_reference.py:

  * feat_generic   pp_feat_generic_fwd / pp_feat_generic_bwd_k0 (csrc/pp_color.hip)
  * mlp            pp_mlp_fwd / pp_mlp_bwd (layer by layer, fp32-fused and split-precision fused routes)
  * pick_rows      input selection for the MLP tests, decided by the float64 reference alone

Run in float64 they are the yardstick of tests/test_hip_generic_kernels.py, run in float32 they give the error of a
straightforward fp32 evaluation of the same maths; tests/test_generic_reference.py pins them to stage_reference.color_feat and to
the torch.nn.Sequential the twin builds.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests.stage_reference import _leaf, _t, grid_u


def feat_generic(k0, pts, viewdirs, ray_id, gradient, pe_w, sel, k0_skip, ld, Lp, Lv, xyz_min, xyz_max, dtype=torch.float64,
                 feat_grad=None, k0_raw_grad=None):
    """[k0 lookup without its first k0_skip channels | x, sin(2^k x), cos(2^k x) | v, sin, cos | normal] padded with zeros to
    `ld` columns, and the full lookup k0_raw [M,C].  k0 is [C,X,Y,Z]; the lookup is trilinear, align_corners, zeros outside the
    grid; x = (p - xyz_min) / (xyz_max - xyz_min), v the viewdir of the sample's ray; sin / cos blocks are axis-major
    (column a * L + k), weighted by pe_w = [position (Lp) | view (Lv)] when given; normal = g / (|g| + 1e-5), present only when
    `gradient` is given.  Rows with sel == 0 are zero in both outputs (sel None: every row takes part).
    With feat_grad [M,ld] (and optionally k0_raw_grad [M,C]): the autograd gradient of <feat, feat_grad> + <k0_raw, k0_raw_grad>
    with respect to k0, dense [C,X,Y,Z]."""
    M = pts.shape[0]
    k0 = _leaf(k0, dtype)
    p = _t(pts, dtype)
    vs = _t(torch.as_tensor(viewdirs)[torch.as_tensor(ray_id).long()], dtype)
    mn, mx = _t(xyz_min, dtype), _t(xyz_max, dtype)
    C = k0.shape[0]
    coords = ((p - mn) / (mx - mn)).flip((-1,)) * 2 - 1
    kf = F.grid_sample(k0[None], coords.reshape(1, 1, 1, M, 3), mode='bilinear', align_corners=True, padding_mode='zeros')
    kf = kf.reshape(C, M).T

    def enc(x, L, w):
        freq = torch.tensor([2. ** i for i in range(L)], dtype=dtype)
        emb = (x.unsqueeze(-1) * freq).flatten(-2)
        w3 = torch.ones(3 * L, dtype=dtype) if w is None else w.repeat(3)
        return torch.cat([x, emb.sin() * w3, emb.cos() * w3], -1)

    pw = None if pe_w is None else _t(pe_w, dtype)
    x = (p - mn) / (mx - mn)
    cols = [kf[:, k0_skip:], enc(x, Lp, None if pw is None else pw[:Lp]), enc(vs, Lv, None if pw is None else pw[Lp:Lp + Lv])]
    if gradient is not None:
        g = _t(gradient, dtype)
        cols.append(g / (g.norm(dim=-1, keepdim=True) + 1e-5))
    feat = torch.cat(cols, -1)
    width = feat.shape[1]
    assert width <= ld, (width, ld)
    feat = F.pad(feat, (0, ld - width))
    on = torch.ones(M, 1, dtype=dtype) if sel is None else _t(np.asarray(sel) != 0, dtype).reshape(M, 1)
    feat, k0_raw = feat * on, kf * on
    out = {'feat': feat.detach(), 'k0_raw': k0_raw.detach(), 'width': width}
    if feat_grad is not None:
        L = (feat * _t(feat_grad, dtype)).sum()
        if k0_raw_grad is not None:
            L = L + (k0_raw * _t(k0_raw_grad, dtype)).sum()
        out['k0_grad'] = torch.autograd.grad(L, [k0])[0]
    return out


def corner_absmax(k0, pts, xyz_min, xyz_max):
    """Largest |k0| over the (in-grid) corners of each point's voxel cell and all channels, [M,1] float64: the size of the terms
    of a row's trilinear sums.  Points are expected off integer voxel coordinates or exactly on a face."""
    k0 = np.abs(np.asarray(k0, np.float64))
    size = np.array(k0.shape[1:])
    u = grid_u(np.asarray(pts, np.float64), np.asarray(xyz_min, np.float64), np.asarray(xyz_max, np.float64), size.astype(np.float64))
    f = np.floor(u).astype(np.int64)
    out = np.zeros((len(u), 1))
    k0max = k0.max(0)
    for d in np.ndindex(2, 2, 2):
        i = f + np.array(d)
        ok = ((i >= 0) & (i < size)).all(-1)
        ic = np.clip(i, 0, size - 1)
        out[:, 0] = np.maximum(out[:, 0], np.where(ok, k0max[ic[:, 0], ic[:, 1], ic[:, 2]], 0.0))
    return out


# ------------------------------------------------------------------------------------------------------------------ MLP
def mlp_params(width, n_gemm, seed):
    """[(W, b)] of width -> 128 x n_gemm -> 3 with the initialisation of tests/test_hip_mlp.py::_rgb_params (float32)."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(128, width)] + [(128, 128)] * (n_gemm - 1) + [(3, 128)]
    return [(torch.randn(o, k, generator=g) * (1.4 / np.sqrt(k)), torch.randn(o, generator=g) * 0.1) for o, k in shapes]


def mlp(params_layers, feat, logit_add=None, dtype=torch.float64, out_grad=None):
    """ReLU hidden layers, a 128 -> 3 output, the first three columns of logit_add added to the logits, sigmoid.  feat is
    [M, >= width]: the columns past the first layer's width are ignored.  Returns out, the logits and every hidden
    pre-activation (`pre`); with out_grad [M,3] also the autograd gradients of all weights and biases (`params_grad`, as
    [(gW, gb)]), of feat (`feat_grad`, [M,width]) and of the logits (`logit_grad`, which is also logit_add's gradient)."""
    lay = [(_leaf(W, dtype), _leaf(b, dtype)) for W, b in params_layers]
    width = lay[0][0].shape[1]
    x = _leaf(torch.as_tensor(feat)[:, :width], dtype)
    h, pre = x, []
    for W, b in lay[:-1]:
        y = h @ W.T + b
        pre.append(y)
        h = torch.relu(y)
    z = torch.zeros(x.shape[0], 3, dtype=dtype, requires_grad=True)          # a leaf added to the logits: its gradient is theirs
    logits = h @ lay[-1][0].T + lay[-1][1] + z
    if logit_add is not None:
        logits = logits + _t(torch.as_tensor(logit_add)[:, :3], dtype)
    out = torch.sigmoid(logits)
    res = {'out': out.detach(), 'logits': logits.detach(), 'pre': [y.detach() for y in pre]}
    if out_grad is not None:
        leaves = [t for Wb in lay for t in Wb] + [x, z]
        gs = torch.autograd.grad((out * _t(out_grad, dtype)).sum(), leaves)
        res.update(params_grad=[(gs[2 * i], gs[2 * i + 1]) for i in range(len(lay))], feat_grad=gs[-2], logit_grad=gs[-1])
    return res


def clear_rows(candidates, layers):
    """Boolean [N]: rows in which every float64 hidden pre-activation y satisfies |y| >= 1e-5 * max(1, max |y| of that row and
    layer), so that no ReLU sits within fp32 rounding of zero."""
    pre = mlp(layers, candidates)['pre']
    ok = torch.ones(len(candidates), dtype=torch.bool)
    for y in pre:
        ok &= (y.abs() >= 1e-5 * y.abs().amax(1, keepdim=True).clamp_min(1.0)).all(1)
    return ok


def pick_rows(candidates, layers, M):
    """The first M rows of `candidates` that clear_rows keeps (decided by the float64 reference alone, never by a kernel)."""
    ok = clear_rows(candidates, layers)
    assert int(ok.sum()) >= M, f'only {int(ok.sum())} of {len(candidates)} candidate rows are clear of a ReLU edge, {M} needed'
    return torch.as_tensor(candidates)[ok.nonzero()[:M, 0]]


def mlp_inputs(width, n_gemm, M, seed):
    """(layers, feat [M,width]): the parameters of mlp_params(seed) and M rows picked from ceil(1.1 M) standard-normal candidates."""
    layers = mlp_params(width, n_gemm, seed)
    g = torch.Generator().manual_seed(seed + 1000 + M)
    cand = torch.randn(int(np.ceil(1.1 * M)), width, generator=g)
    return layers, pick_rows(cand, layers, M)
