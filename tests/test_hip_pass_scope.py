"""RenderCore.pass_scope: the weight-pack record and the lean scope of a render pass are dropped when the pass raises on the host,
so that the next caller of the forward kernels with the same parameter pointers reads the CURRENT weights and writes every
activation row.  The exception is a Python one raised before a launch: nothing faults on the device."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

G, V, H, W, N, ROWS, MATCHED, GS = 24, 3, 16, 16, 64, 32, 16, 10


def _engine():
    """24^3 voxels, 3 views of 16 x 16, 64 rays, 32 reprojection rows; a private context with the library's default option values
    (the host's shared default context is never involved).  One good step is run."""
    from oracle import voxurf_oracle as O
    from poseprobe_amd import _lib
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    rs = syn.range_shape()
    views = syn.make_views(V, H, W)
    scene = O.Scene(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, output_range=float(rs.max()), rect_size=rs.tolist())
    P = O.init_params(scene, seed=2)
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max()))
    eng = TrainEngine(cfg, V, H, W, N, device='cuda:0', reproj_rows=ROWS,
                      options={k: _lib.library_default(k) for k in _lib.OPTION_NAMES})
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    eng.zero_grads()
    idx, jit = syn.step_randomness(V * H * W, N, seed=1)
    step = (torch.tensor(idx, dtype=torch.int32, device='cuda:0'), torch.tensor(jit, device='cuda:0'), GS)
    eng.train_step(*step)
    return eng, step


def _rows(dev='cuda:0'):
    g = torch.Generator().manual_seed(3)
    own = torch.randint(0, V, (MATCHED,), generator=g)
    px = lambda: (torch.rand(MATCHED, 2, generator=g) * torch.tensor([W - 1., H - 1.])).to(dev)
    return dict(own=own.to(torch.int32).to(dev), other=((own + 1) % V).to(torch.int32).to(dev), pix=px(), match=px(),
                conf=torch.rand(MATCHED, generator=g).to(dev))


def _forward_twice(eng, ws, jitter):
    """The forward chain on `ws` straight after the failed pass, then again after dropping every record of the context by hand
    -> must be the same bits: the first run saw no stale record."""
    from poseprobe_amd import ops
    P = eng.flat
    inv_s = float(np.float32(1.0) / np.float32(eng.cfg.s_val(GS)))
    with torch.no_grad():
        P.view('warp').mul_(0.5)                                    # in place: same pointer, new values
    got = []
    for drop in (False, True):
        if drop:
            ops.mlp_pack_invalidate(eng.ctx)
            ops.warp_lean_end(eng.ctx)
        ws.warp_acts.zero_()
        eng.core.sample(ws, jitter)
        eng.core.forward(ws, eng.k0_cl, eng.sdf, P.view('sdf_ab'), P.view('rgbnet'), P.view('warp'), inv_s, eng.pe_w)
        torch.cuda.synchronize()
        got.append((ws.warp_out.clone(), ws.warp_acts.clone()))
    assert int(ws.count.item()) > N                                 # more than one 64-row tile of samples
    # bit patterns, not values: warp_out's rows past the samples are never written, and whatever the allocator left there (NaN
    # included, which no value comparison calls equal to itself) is the same in both runs
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(got[0][0], got[1][0]), 'warp_out: the forward after the failed pass read a pack of the old weights'
    assert same(got[0][1], got[1][1]), 'warp_acts: the forward after the failed pass ran inside a stale lean scope'


def _boom(*a, **k):
    raise RuntimeError('host-side failure inside the pass')


def test_scope_is_closed_when_the_step_raises(monkeypatch):
    from poseprobe_amd import ops
    eng, step = _engine()
    with monkeypatch.context() as m:
        m.setattr(ops, 'loss_rays', _boom)
        with pytest.raises(RuntimeError, match='host-side failure'):
            eng.render_and_grads(*step)
    _forward_twice(eng, eng.ws, step[1])


def test_scope_is_closed_when_the_reprojection_pass_raises(monkeypatch):
    from poseprobe_amd import ops
    eng, step = _engine()
    jitter = torch.rand(ROWS, generator=torch.Generator().manual_seed(4)).to('cuda:0')
    with monkeypatch.context() as m:
        m.setattr(ops, 'reproj_loss', _boom)
        with pytest.raises(RuntimeError, match='host-side failure'):
            eng.reprojection_grads(_rows(), 'render', GS, jitter=jitter)
    _forward_twice(eng, eng.ws_reproj, jitter)
