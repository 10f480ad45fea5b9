"""GPU test of the loss-gradient bookkeeping of bg_nerf.SceneEngine.forward_backward: one engine keeps g_rgb (zero on the matched
tail) and g_depth (zero on the photometric prefix) per pass across calls whose split between photometric and matched rows
changes; a call must see exact zeros where it expects them, whatever the calls before it left behind."""
import pytest
import torch

from tests.test_hip_scene_deterministic import NF, _nets, _opt

pytestmark = pytest.mark.gpu

R, S = 40, 16
RANGE = (0.4, 2.4)


def _rows(M, seed):
    """CorresRows of M matched pixels of a view pair: the last 2M of the R rows."""
    from poseprobe_amd import bg_nerf
    g = torch.Generator().manual_seed(seed)
    K = torch.tensor([[60., 0., 32.], [0., 60., 24.], [0., 0., 1.]]).cuda()
    w2c = torch.eye(3, 4)[None].repeat(2, 1, 1)
    w2c[1, 0, 3] = 0.2
    w2c = w2c.cuda()
    pix = (torch.rand(2, M, 2, generator=g) * torch.tensor([63., 47.])).cuda()
    return bg_nerf.CorresRows(pix[0], pix[1], torch.rand(M, generator=g).cuda(), K, K, w2c[0], w2c[1], 1e-2,
                              fine_grid=torch.rand(NF + 1, generator=g))


def _bits(t):
    return t.detach().clone().view(torch.int32)


def test_loss_gradient_buffers_are_clean_for_every_split():
    """One deterministic engine (coarse + fine network), R = 40 rows, four forward_backward calls - matched rows M = 4 (Rp = 32),
    plain (Rp = 40), M = 6 (Rp = 28), M = 4 again - with the gradient blocks zeroed in between and no optimiser step.  After
    each, the same call on a freshly built engine with identical network state: both networks' gradient blocks, the returned
    g_center / g_ray and last_g_w2c equal bit for bit."""
    from poseprobe_amd import bg_nerf
    g = torch.Generator().manual_seed(29)
    center, ray = (torch.randn(R, 3, generator=g) * 0.3).cuda(), torch.randn(R, 3, generator=g).cuda()
    depth = ((torch.rand(R, S, generator=g) + torch.arange(S)) / S * (RANGE[1] - RANGE[0]) + RANGE[0]).cuda().contiguous()
    image = torch.rand(R, 3, generator=g).cuda()
    grid = torch.rand(NF + 1, generator=g)

    def call(eng, M):
        kw = dict(fine=True, depth_range=RANGE, fine_grid=grid)
        if M:
            kw['corres'] = _rows(M, seed=M)
        for st in eng.states:
            st.grad.zero_()
        _, gc, gr = eng.forward_backward(center, ray, depth, image[:R - 2 * M].contiguous(), **kw)
        torch.cuda.synchronize()
        out = {f'net{i}.grad': _bits(st.grad) for i, st in enumerate(eng.states)}
        out.update(g_center=_bits(gc), g_ray=_bits(gr))
        if M:
            out['g_w2c'] = _bits(eng.last_g_w2c)
        return out

    net, net_f = _nets(_opt(S))
    old = bg_nerf.SceneEngine(net, net_fine=net_f, deterministic=True)
    for n, M in enumerate((4, 0, 6, 4)):
        net, net_f = _nets(_opt(S))
        # identical network state: the same seeded construction, and no optimiser step has moved the used engine's
        assert torch.equal(net.flat, old.net.flat) and torch.equal(net_f.flat, old.net_fine.flat)
        fresh = bg_nerf.SceneEngine(net, net_fine=net_f, deterministic=True)
        a, b = call(old, M), call(fresh, M)
        assert a.keys() == b.keys()
        for k in a:
            assert bool((a[k] != 0).any()), f'call {n + 1} (M = {M}): {k} is all zero'
            assert torch.equal(a[k], b[k]), (f'call {n + 1} (M = {M}): {k} of the used engine differs from a fresh engine\'s in '
                                             f'{int((a[k] != b[k]).sum())} of {a[k].numel()} entries')
