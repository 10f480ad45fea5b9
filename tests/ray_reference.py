"""Plain-autograd references of the first kernels of an object-branch step, parameterised by dtype (CPU, torch): the pose chain
with its Jacobian (pp_pose_fwd / pp_pose_bwd) and the two loss kernels (pp_loss_rays / pp_loss_samples).

Run in float64 they are the yardstick of tests/test_hip_ray_kernels.py; run in float32 they give the error a straightforward fp32
evaluation of the same maths makes.  tests/test_ray_reference.py pins them to the pose fixture and to the oracle's object_losses.
Nothing here restates the kernels' hand derivations: the pose Jacobian and every loss gradient come from torch.autograd.
"""
import numpy as np
import torch

from oracle import voxurf_oracle as O

F32 = np.float32
# the clamp bounds of object_losses as the fp32 program sees them: float32 values, the upper ones subtracted in float32
ENT_LO, ENT_HI = float(F32(1e-6)), float(F32(1) - F32(1e-6))
BCE_LO, BCE_HI = float(F32(1e-3)), float(F32(1) - F32(1e-3))
W_EIKONAL = 1.0                                       # object_losses: Wt['grad_constraint']


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)).to(dtype).clone()


def _leaf(x, dtype):
    return _t(x, dtype).requires_grad_(True)


# ------------------------------------------------------------------------------------------------------------------------- pose
def pose_chain(se3, w2c_init, refine_mask=None, dtype=torch.float64):
    """se3 [V,6], w2c_init [V,3,4], refine_mask [V] or None -> w2c [V,3,4], c2w [V,3,4], jac [V,12,6] = d c2w / d se3.

    w2c = se3_to_SE3(se3) composed onto w2c_init, c2w its inverse, both by the oracle's own functions; views with
    refine_mask == 0 keep w2c_init and have a zero Jacobian.  The views do not interact, so the Jacobian of the sum of c2w over the
    views (12 backward passes) holds every view's own [12,6] block.  Meant for |w| <= 3: the first term the 11-term series of the
    oracle (and of the kernel) drops is then below 1e-10."""
    se3 = _t(se3, dtype)
    init = _t(w2c_init, dtype)
    V = se3.shape[0]
    fixed = None if refine_mask is None else (torch.as_tensor(np.asarray(refine_mask)) == 0)[:, None, None]

    def chain(s):
        w2c = O.pose_compose_pair(O.se3_to_SE3(s), init)
        if fixed is not None:
            w2c = torch.where(fixed, init, w2c)
        return w2c, O.pose_invert(w2c)

    w2c, c2w = chain(se3)
    assert w2c.dtype == c2w.dtype == dtype
    jac = torch.autograd.functional.jacobian(lambda s: chain(s)[1].reshape(V, 12).sum(0), se3)          # [12, V, 6]
    return w2c, c2w, jac.permute(1, 0, 2).contiguous()


def pose_term_scale(se3, w2c_init):
    """[V] the largest term of the sums behind a view's w2c / c2w / jac entries: the series terms t^i / (2i+1)! ... times |w| or
    |w|^2 (they cancel to sin / cos at |w| = 3, where single terms reach 4.5), and for the translation column |V u| + |t_init|."""
    se3, init = np.asarray(se3, np.float64), np.asarray(w2c_init, np.float64)
    th = np.linalg.norm(se3[:, :3], axis=1)
    fact = np.cumprod(np.arange(1, 24, dtype=np.float64))                       # fact[n - 1] = n!
    a, b, c = (np.max(np.stack([th ** (2 * i) / fact[2 * i + off - 1] for i in range(11)]), 0) for off in (1, 2, 3))
    rot = np.maximum(1.0, np.maximum(a * th, b * th ** 2))
    vm = np.maximum(1.0, np.maximum(b * th, c * th ** 2))
    trans = vm * np.linalg.norm(se3[:, 3:], axis=1) + np.linalg.norm(init[:, :, 3], axis=1)
    return rot * np.maximum(1.0, trans)


# ----------------------------------------------------------------------------------------------------------------------- losses
def ray_losses(rgb_marched, alphainv_last, cum_weights, target, mask, w_main, w_entropy, w_mask, loss_scale,
               dtype=torch.float64, batch_norm=None):
    """The ray-level terms of object_losses for N rays (rgb_marched, target [N,3]; alphainv_last, cum_weights, mask [N], given as
    float32 values): masked MSE / (sum(mask) * 3), entropy of clamp(alphainv_last), BCE of clamp(cum_weights) against the mask,
    the last two as means over the rays.  batch_norm = (masked pixels, samples) of a larger batch: the MSE is then normalised by
    batch_norm[0] * 3.  -> dict(mse, entropy, bce, total [the weighted sum], mask_sum, g_rgbm, g_last, g_cw [gradients of
    loss_scale * total])."""
    rgbm, a, cw = _leaf(rgb_marched, dtype), _leaf(alphainv_last, dtype), _leaf(cum_weights, dtype)
    tgt, y = _t(target, dtype), _t(mask, dtype).reshape(-1)
    msum = y.sum()
    norm = msum if batch_norm is None else _t(batch_norm, dtype)[0]
    mse = ((rgbm * y[:, None] - tgt * y[:, None]) ** 2).sum() / (norm * 3)
    p = a.clamp(ENT_LO, ENT_HI)
    entropy = -(p * torch.log(p) + (1 - p) * torch.log(1 - p)).mean()
    c = cw.clamp(BCE_LO, BCE_HI)
    bce = -(y * torch.log(c) + (1 - y) * torch.log(1 - c)).mean()
    total = w_main * mse + w_entropy * entropy + w_mask * bce
    g = torch.autograd.grad(total * loss_scale, (rgbm, a, cw))
    return dict(mse=mse.detach(), entropy=entropy.detach(), bce=bce.detach(), total=total.detach(), mask_sum=msum,
                g_rgbm=g[0], g_last=g[1], g_cw=g[2])


def sample_losses(gradient, grad_deform, warp_out, sdf_deform, count, w_eikonal, w_deform, loss_scale, dtype=torch.float64,
                  batch_norm=None):
    """The sample-level terms of object_losses on the first M = min(count, rows) rows (gradient [.,3], grad_deform [.,9] = three
    rows of three, warp_out [.,16] whose column 3 is the SDF correction, sdf_deform [.]): eikonal mean | |gradient| - 1 |, mean
    row norm of grad_deform, mean |correction|, mean |sdf_deform|.  With batch_norm the sums are divided by batch_norm[1] (the row
    norms by 3 * batch_norm[1]) instead of M.  -> dict(eikonal, grad_deform, correction, sdf_deform, total, M, g_gradient [M,3],
    g_grad_deform [M,9], g_correction [M], g_sdf_deform [M]); everything zero / empty for M = 0."""
    M = max(0, min(int(count), len(gradient)))
    z = torch.zeros((), dtype=dtype)
    if M == 0:
        e = lambda *s: torch.zeros(0, *s, dtype=dtype)
        return dict(eikonal=z, grad_deform=z, correction=z, sdf_deform=z, total=z, M=0, g_gradient=e(3), g_grad_deform=e(9),
                    g_correction=e(), g_sdf_deform=e())
    g, gd = _leaf(np.asarray(gradient)[:M], dtype), _leaf(np.asarray(grad_deform)[:M], dtype)
    corr, sd = _leaf(np.asarray(warp_out)[:M, 3], dtype), _leaf(np.asarray(sdf_deform)[:M], dtype)
    n = float(M) if batch_norm is None else _t(batch_norm, dtype)[1]
    eikonal = torch.abs(g.norm(dim=-1) - 1).sum() / n
    l_gd = gd.reshape(M, 3, 3).norm(dim=-1).sum() / (n * 3)
    l_c = torch.abs(corr).sum() / n
    l_sd = torch.abs(sd).sum() / n
    total = w_eikonal * eikonal + w_deform * (l_gd + l_c + l_sd)
    gr = torch.autograd.grad(total * loss_scale, (g, gd, corr, sd))
    return dict(eikonal=eikonal.detach(), grad_deform=l_gd.detach(), correction=l_c.detach(), sdf_deform=l_sd.detach(),
                total=total.detach(), M=M, g_gradient=gr[0], g_grad_deform=gr[1], g_correction=gr[2], g_sdf_deform=gr[3])
