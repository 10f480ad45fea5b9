"""Plain references of the optimiser and total-variation kernels, parameterised by dtype (CPU, torch).

Written from the reference model's expressions - total_variation (sum of |forward differences| along the three grid axes),
its autograd gradient, and Adam with bias corrections (no weight decay, no amsgrad) - not from the kernels: no chunks, no
marching, no float4.  Run in float64 they are the yardstick of tests/test_hip_optim_kernels.py; run in float32 they give the
error a straightforward fp32 evaluation of the same maths makes, from which that file's tolerances are taken
(tests/test_optim_reference.py pins both).

Layout follows the kernels: the grid is channels-last [X,Y,Z,C]; a `touched` map is [X,Y,Z] (or flat), non-zero = marked.
Scalars (learning rate, betas, eps, scales) are used as given, in double precision: a caller that wants the numbers the C ABI
carries passes them already rounded to float32.
"""
import math

import torch


def _t(x, dtype):
    return torch.as_tensor(x).detach().cpu().to(dtype).clone()


def _fwd_diffs(p, x_begin=0, x_end=None):
    """|forward differences| owned by the voxels of planes [x_begin, x_end): the +x difference of plane x belongs to plane x
    (so the one between x_end - 1 and x_end counts whenever x_end < X), the +y / +z ones stay inside their plane."""
    X = p.shape[0]
    x_end = X if x_end is None else x_end
    s = p[x_begin:x_end]
    dx = (p[x_begin + 1:min(x_end, X - 1) + 1] - p[x_begin:min(x_end, X - 1)]).abs()
    dy = (s[:, 1:] - s[:, :-1]).abs()
    dz = (s[:, :, 1:] - s[:, :, :-1]).abs()
    return dx, dy, dz


def tv_value(p, dtype=torch.float64):
    """Sum (not mean: dividing by 3 * numel is the caller's job) of |forward differences| of p [X,Y,Z,C] along x, y and z."""
    p = torch.as_tensor(p).to(dtype)
    dx, dy, dz = _fwd_diffs(p)
    return dx.sum() + dy.sum() + dz.sum()


def tv_grad(p, dtype=torch.float64):
    """d tv_value / d p by autograd; abs has derivative 0 at 0, which is the sgn 0 = 0 convention."""
    p = _t(p, dtype).requires_grad_(True)
    return torch.autograd.grad(tv_value(p, dtype), p)[0]


def _adam(p, g, m, v, lr, beta1, beta2, eps, step):
    """One Adam step, out of place; lr is a number or a tensor broadcast against p."""
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    m = m * beta1 + (1 - beta1) * g
    v = v * beta2 + (1 - beta2) * g * g
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def grid_step(p, grad, m, v, x_begin, x_end, tv_scale, grad_scale, lr, beta1, beta2, eps, step, touched=None,
              dtype=torch.float64):
    """pp_grid_tv_adam_step{,_sparse} on the slab [x_begin, x_end) of the channels-last grid: the gradient of every slab voxel
    is grad_scale * grad + tv_scale * tv_grad(p) (neighbours taken from the WHOLE grid), then Adam, then the gradient is
    zero-filled.  With a `touched` map the data gradient of an unmarked voxel counts as 0 and is left as it was; a marked
    voxel's gradient is zero-filled.  Returns (p_out, m, v, grad_after, tv_slab); everything outside the slab is returned
    unchanged (p_out equals p there), tv_slab is the sum of the |forward differences| the slab's voxels own."""
    p, grad, m, v = (_t(a, dtype) for a in (p, grad, m, v))
    X, Y, Z, C = p.shape
    marked = torch.ones(X, Y, Z, dtype=torch.bool) if touched is None else torch.as_tensor(touched).cpu().reshape(X, Y, Z) != 0
    g = grad_scale * torch.where(marked[..., None], grad, torch.zeros_like(grad)) + tv_scale * tv_grad(p, dtype)
    sl = slice(x_begin, x_end)
    p_out, m_out, v_out, grad_after = p.clone(), m.clone(), v.clone(), grad.clone()
    p_out[sl], m_out[sl], v_out[sl] = _adam(p[sl], g[sl], m[sl], v[sl], lr, beta1, beta2, eps, step)
    grad_after[sl] = torch.where(marked[sl][..., None], torch.zeros_like(grad[sl]), grad[sl])
    tv_slab = sum(d.sum() for d in _fwd_diffs(p, x_begin, x_end))
    return p_out, m_out, v_out, grad_after, tv_slab


def segment_lr(n, seg_end, seg_lr, dtype=torch.float64):
    """Per-element learning rate of a packed buffer: element i belongs to the first segment whose end exceeds i; elements
    past the last end take the last learning rate."""
    seg_end = [int(e) for e in torch.as_tensor(seg_end).reshape(-1)]
    seg_lr = _t(seg_lr, dtype).reshape(-1)
    lr = seg_lr[-1].repeat(n)
    begin = 0
    for e, r in zip(seg_end, seg_lr):
        lr[begin:min(e, n)] = r
        begin = e
    return lr


def adam_flat(p, grad, m, v, seg_end, seg_lr, grad_scale, beta1, beta2, eps, step, zero_grad, dtype=torch.float64):
    """pp_adam_flat: Adam on grad_scale * grad with per-segment learning rates.  lr == 0 leaves p untouched and still updates
    both moments.  Returns (p, m, v, grad_after)."""
    p, grad, m, v = (_t(a, dtype) for a in (p, grad, m, v))
    lr = segment_lr(p.numel(), seg_end, seg_lr, dtype)
    p_new, m, v = _adam(p, grad_scale * grad, m, v, lr, beta1, beta2, eps, step)
    return torch.where(lr != 0, p_new, p), m, v, (torch.zeros_like(grad) if zero_grad else grad)
