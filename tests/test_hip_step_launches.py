"""The train step's head launch (pp_step_begin) and its fused ray launch (pp_march_loss_bwd) at engine level: the default
step against the same step on the separate launches.  The separate launches are selected with the constructor switches
TrainEngine(fuse_head=False, fuse_rays=False); nothing is monkeypatched but the call recorder of the last test.

Two engines are driven in lockstep: both take the same step from the SAME state (the second engine's trainable state is overwritten
with the first one's after every step), so that everything a step computes without float atomics can be compared bit for bit at
every step, not only at the first.  That covers everything the two new launches write (poses, Jacobian, step scalars, weight pack,
every compositing output, every ray-loss gradient, g_alpha, g_rgb).  What follows the atomic sums of the backward (parameter
gradients of both MLPs, the k0 scatter, c2w_grad) differs from run to run on EITHER route; its bounds are written where they are
used.
"""
import numpy as np
import pytest
import torch

from tests import optim_cases as K
from tests.helpers import assert_close
from tests.test_hip_side_by_side import EPS, same_bits, small_engine

pytestmark = pytest.mark.gpu

STATE = ('k0_m', 'k0_v', 'k0_grad', 'k0_touched', 'se3', 'se3_m', 'se3_v', 'se3_grad', 'c2w_grad')
FLAT = ('data', 'grad', 'm', 'v')
EXACT_ENGINE = ('w2c', 'c2w', 'jac', 'step_dev', 'mlp_pack')
EXACT_RAYS = ('alphainv_last', 'i_end', 'rgb_marched', 'rgb_pre', 'cum_weights', 'depth_acc', 'g_rgbm', 'g_last', 'g_cw', 'mask_sum')
EXACT_SAMPLES = ('alpha', 'rgb', 'weights', 'T', 'g_alpha', 'g_rgb')


def adopt_state(dst, src):
    """dst's trainable state := src's (both went through the same host logic: learning rates, step counters and buffer parities agree)."""
    assert (dst.k0_cur, dst.touch_par, dst.n_step, dst.lr, dst.lr_pose) == (src.k0_cur, src.touch_par, src.n_step, src.lr, src.lr_pose)
    with torch.no_grad():
        for i in range(2):
            dst.k0[i].copy_(src.k0[i])
        for k in STATE:
            getattr(dst, k).copy_(getattr(src, k))
        for k in FLAT:
            getattr(dst.flat, k).copy_(getattr(src.flat, k))


def compare_exact(a, b, what):
    for k in EXACT_ENGINE:
        same_bits(getattr(a, k), getattr(b, k), f'{what}: {k}')
    M = int(a.ws.count.item())
    assert M == int(b.ws.count.item()) and M > 256
    for k in EXACT_RAYS:
        same_bits(getattr(a.ws, k), getattr(b.ws, k), f'{what}: {k}')
    for k in EXACT_SAMPLES:
        same_bits(getattr(a.ws, k)[:M], getattr(b.ws, k)[:M], f'{what}: {k}')


def compare_after_atomics(a, b, what):
    """Both routes add the same terms with float atomics in an order of their own.
    loss_out: sums of non-negative terms, in trees and atomic chains of well under 64 additions on either route - 64 float32 ulps of
    the value, the figure the side-by-side tests use for such sums.  tv_out: optim_cases.TOL['grid.tv'], as there.
    Parameters: Adam moves an element by at most lr * max(1, (1 - b1) / sqrt(1 - b2)) per step whatever its gradients were (Kingma &
    Ba, section 2.1) - an element whose gradient is rounding noise around zero may take that step in opposite directions on the two
    routes; both start the step from the same value and moments, so they end at most two such steps apart (the factor 1.06 covers
    eps and the float32 rounding of the update).
    Moments: the parameter-gradient tolerance of tests/test_hip_mlp_pack.py for float atomic sums, 2e-5 + 1e-3 |x| + 1e-3 max |x|,
    which m = b1 m + (1 - b1) g and v = b2 v + (1 - b2) g^2 inherit from g with factors below one."""
    la, lb = a.ws.loss_out.double().cpu(), b.ws.loss_out.double().cpu()
    assert bool((lb > 0).all()) and bool(((la - lb).abs() <= 64 * EPS * lb.abs()).all()), f'{what}: loss_out {la} {lb}'
    assert_close(a.ws.tv_out.cpu(), b.ws.tv_out.cpu().double(), atol=0.0, name=f'{what} tv_out', **K.TOL['grid.tv'])

    def close(x, y, name):
        x, y = x.double().cpu(), y.double().cpu()
        bound = 2e-5 + 1e-3 * y.abs() + 1e-3 * y.abs().max()
        assert bool(((x - y).abs() <= bound).all()), f'{what}: {name} max |difference| {float((x - y).abs().max()):.3e}'

    def step_bound(lr, b1, b2):
        return 2 * 1.06 * lr * max(1.0, (1 - b1) / np.sqrt(1 - b2))

    for name, (o, n) in a.flat.off.items():
        lr = a.lr[name]
        d = (a.flat.data[o:o + n].double() - b.flat.data[o:o + n].double()).abs().max().item()
        assert d <= step_bound(lr, 0.9, 0.99), f'{what}: {name} parameters {d:.3e}'
    assert (a.k0_cl.double() - b.k0_cl.double()).abs().max().item() <= step_bound(a.lr['k0'], 0.9, 0.99), f'{what}: k0'
    assert (a.se3.double() - b.se3.double()).abs().max().item() <= step_bound(a.lr_pose / a.pose_gamma, 0.9, 0.999), f'{what}: se3'
    for k in ('m', 'v'):
        close(getattr(a.flat, k), getattr(b.flat, k), f'flat.{k}')
        close(getattr(a, 'k0_' + k), getattr(b, 'k0_' + k), f'k0_{k}')
        close(getattr(a, 'se3_' + k), getattr(b, 'se3_' + k), f'se3_{k}')
    assert float(a.flat.grad.abs().max()) == 0.0 and float(a.se3_grad.abs().max()) == 0.0 and float(a.c2w_grad.abs().max()) == 0.0


def test_three_default_steps_against_the_separate_launches():
    new, idx, jit = small_engine()
    old, _, _ = small_engine(fuse_head=False, fuse_rays=False)
    assert new.ray_work is not None and new.side_by_side and old.side_by_side
    for e in (new, old):
        e.mlp_pack.zero_()                     # the pack has scalar slots that nobody writes: the same fill in both
    packs = []
    for s in range(3):
        new.train_step(idx, jit, 10 + s)
        old.train_step(idx, jit, 10 + s)
        torch.cuda.synchronize()
        compare_exact(new, old, f'step {s}')
        compare_after_atomics(new, old, f'step {s}')
        assert int(new.ray_work.view(torch.int32)[0]) == 0, 'ticket of the fused ray launch not left zero'
        packs.append(new.mlp_pack.clone())
        adopt_state(old, new)
    # the optimiser moved the weights between the steps, and every step packed its own
    assert not torch.equal(packs[0], packs[1]) and not torch.equal(packs[1], packs[2])
    assert float(new.ws.g_alpha.abs().max()) > 0 and float(new.ws.loss_out[0]) > 0 and float(new.ws.tv_out[0]) > 0


def test_a_parameter_write_between_two_steps_is_seen():
    """flat.data.copy_ and se3.copy_ between two steps, from outside the engine: the next step packs and poses from the new values,
    exactly as the separate launches do."""
    from poseprobe_amd import ops
    new, idx, jit = small_engine()
    old, _, _ = small_engine(fuse_head=False, fuse_rays=False)
    for e in (new, old):
        e.mlp_pack.zero_()
        e.train_step(idx, jit, 10)
    adopt_state(old, new)
    with torch.no_grad():
        flat, se3 = new.flat.data * 0.9, new.se3 + 0.01
        for e in (new, old):
            e.flat.data.copy_(flat)
            e.se3.copy_(se3)
    # what the head of the next step has to produce from the written values
    want_pack, want = torch.zeros_like(new.mlp_pack), {k: torch.zeros_like(getattr(new, k)) for k in ('w2c', 'c2w', 'jac')}
    ops.mlp_pack(flat[slice(*_span(new, 'warp'))], flat[slice(*_span(new, 'rgbnet'))], want_pack, ops.Context(mlp_pack=1))
    ops.pose_fwd(se3, new.w2c_init, new.refine_mask, want['w2c'], want['c2w'], want['jac'])
    before = (new.mlp_pack.clone(), new.c2w.clone())
    new.train_step(idx, jit, 11)
    old.train_step(idx, jit, 11)
    torch.cuda.synchronize()
    compare_exact(new, old, 'step after the write')
    compare_after_atomics(new, old, 'step after the write')
    same_bits(new.mlp_pack, want_pack, 'weight pack after flat.data.copy_')
    for k in want:
        same_bits(getattr(new, k), want[k], f'{k} after se3.copy_')
    assert not torch.equal(new.mlp_pack, before[0]) and not torch.equal(new.c2w[1:], before[1][1:])


def _span(eng, name):
    o, n = eng.flat.off[name]
    return o, o + n


NEW = {'pp_step_begin', 'pp_march_loss_bwd'}
OLD = {'pp_pose_fwd', 'pp_mlp_pack', 'pp_march_fwd', 'pp_loss_rays', 'pp_march_bwd'}
KEPT = {'pp_grid_tv_adam_step_tail', 'pp_geometry_color_feat_fwd'}


def test_only_the_default_step_takes_the_two_launches(monkeypatch):
    """Calls counted through a recorder around _lib.call: the default step makes the two new calls once each and none of the five they
    replace; each switch on its own brings its launches back; deterministic=True, pass_scope + core.forward on their own, pose_fwd and
    _upload_step_scalars called directly keep the old calls."""
    from poseprobe_amd import _lib, ops
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, 'call', lambda name, *a: (names.append(name), real(name, *a))[1])

    eng, idx, jit = small_engine()
    names.clear()
    eng.train_step(idx, jit, 10)
    torch.cuda.synchronize()
    assert all(names.count(n) == 1 for n in NEW | KEPT) and not (OLD & set(names)), sorted(set(names))
    assert names[0] == 'pp_step_begin'

    names.clear()
    eng.render_and_grads(idx, jit, 11)                       # other callers of render_and_grads (the joint step) take them as well
    eng.optimizer_step()
    torch.cuda.synchronize()
    assert all(names.count(n) == 1 for n in NEW) and not (OLD & set(names)), sorted(set(names))

    for switch, back, still in (('fuse_head', {'pp_pose_fwd', 'pp_mlp_pack'}, 'pp_march_loss_bwd'),
                                ('fuse_rays', {'pp_march_fwd', 'pp_loss_rays', 'pp_march_bwd'}, 'pp_step_begin')):
        setattr(eng, switch, False)
        names.clear()
        eng.train_step(idx, jit, 12)
        torch.cuda.synchronize()
        assert back <= set(names) and names.count(still) == 1 and not ((OLD - back) & set(names)), (switch, sorted(set(names)))
        setattr(eng, switch, True)

    names.clear()
    P = eng.flat
    with eng.core.pass_scope(P, eng.mlp_pack, eng.ws):
        eng.core.forward(eng.ws, eng.k0_cl, eng.sdf, P.view('sdf_ab'), P.view('rgbnet'), P.view('warp'), 3.0, eng.pe_w)
    ops.pose_fwd(eng.se3, eng.w2c_init, eng.refine_mask, eng.w2c, eng.c2w, eng.jac)
    eng._upload_step_scalars(0.5)
    torch.cuda.synchronize()
    assert {'pp_mlp_pack', 'pp_march_fwd', 'pp_pose_fwd'} <= set(names) and not (NEW & set(names))
    assert np.array_equal(eng.step_dev.cpu().numpy(), eng._step_scalars(0.5))

    names.clear()
    det, idx, jit = small_engine(deterministic=True)
    det.train_step(idx, jit, 10)
    torch.cuda.synchronize()
    assert OLD <= set(names) and not (NEW & set(names)), sorted(set(names))
