"""The weight pack of the object-branch MLPs (pp_mlp_pack, option mlp_pack): kernels that read the pack give bit-identical results
to kernels that derive the same quantities in their prologues, a pack is only ever read for the parameter buffer it was made from,
the pack kernel stays inside its buffer, and TrainEngine re-packs after every kind of parameter write.

Exact comparisons are on the int32 view of the buffers, so that unwritten (NaN-filled) rows compare equal as well.  Parameter
gradients that arrive by float atomics from many work-groups depend on the arrival order in BOTH runs; they are compared at the
tolerance tests/test_hip_mlp.py uses for them, and exactly where at most two work-groups contribute (a + b is commutative).
"""
import numpy as np
import pytest
import torch

from tests.test_hip_mlp import OUT_RANGE, _pack, _rgb_params, _warp_params

pytestmark = pytest.mark.gpu
PAD = 16384                                                     # floats = 64 KB
SENT = 0x7FC0DEAD                                               # a quiet-NaN payload no kernel produces
SIZES = (1, 17, 4096, 54613)                                    # 54613: the sample count of the benchmark step
SCALES = (0.09, 0.005)


def _fenced(n, dev='cuda'):
    arena = torch.empty(n + 2 * PAD, dtype=torch.int32, device=dev).fill_(SENT).view(torch.float32)
    return arena, arena[PAD:PAD + n]


def _intact(arena, n, what):
    a = arena.view(torch.int32)
    assert bool((a[:PAD] == SENT).all()), f'{what}: sentinels IN FRONT of the buffer were overwritten'
    assert bool((a[PAD + n:] == SENT).all()), f'{what}: sentinels BEHIND the buffer were overwritten'


def _same(a, b, name):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{name} differs between mlp_pack = 1 and mlp_pack = 0'


def _atomic_close(a, b, name):
    ga, gb = a.cpu().numpy(), b.cpu().numpy()
    bad = np.abs(ga - gb) > 2e-5 + 1e-3 * np.abs(gb) + 1e-3 * np.abs(gb).max()
    assert bad.sum() == 0, f'{name}: {bad.sum()} entries, max {np.abs(ga - gb).max():.3e}'


def _params(scale, dev='cuda'):
    from poseprobe_amd.engine import pack_rgbnet
    out = []
    for P in (_pack([(W * scale, b * scale) for W, b in _warp_params(3)]), pack_rgbnet([(W * scale, b * scale) for W, b in _rgb_params(5)])):
        t = torch.zeros(P.numel() + 60, device=dev)
        t[:P.numel()] = P.to(dev)
        out.append(t)
    return out                                                  # [warp, rgbnet]


def _run_warp(params, M, ctx):
    from poseprobe_amd import ops
    dev, cap = 'cuda', M
    g = torch.Generator().manual_seed(M + 1)
    pts = (torch.randn(cap, 3, generator=g) * 0.5).to(dev)
    og = torch.randn(cap, 16, generator=g).to(dev)
    count = torch.tensor([M], dtype=torch.int32, device=dev)
    acts = torch.full((4 * cap * 4 * 128,), float('nan'), device=dev)
    out = torch.full((cap, 16), 7.0, device=dev)
    ops.warp_fwd(params, pts, count, cap, OUT_RANGE, acts, out, ctx)
    scratch = torch.zeros(3 * cap * 4 * 128 + 49152, device=dev)
    pgrad = torch.zeros_like(params)
    ptsg = torch.full((cap, 3), 0.25, device=dev)
    ops.warp_bwd(params, pts, acts, og, count, cap, OUT_RANGE, scratch, pgrad, ptsg, ctx)
    torch.cuda.synchronize()
    return dict(out=out, acts=acts, scratch=scratch, pts_grad=ptsg, pgrad=pgrad)


def _run_rgb(params, M, ctx):
    from poseprobe_amd import ops
    dev, cap = 'cuda', M
    g = torch.Generator().manual_seed(M + 2)
    feat = torch.zeros(cap, 64)
    feat[:, :57] = torch.randn(cap, 57, generator=g)
    feat, gr = feat.to(dev), torch.randn(cap, 3, generator=g).to(dev)
    count = torch.tensor([M], dtype=torch.int32, device=dev)
    acts = torch.full((3 * cap * 128,), float('nan'), device=dev)
    rgb = torch.full((cap, 3), 7.0, device=dev)
    ops.rgbnet_fwd(params, feat, count, cap, acts, rgb, ctx)
    scratch = torch.zeros(3 * cap * 128 + 49152, device=dev)
    pgrad = torch.zeros_like(params)
    fgrad = torch.full((cap, 64), 5.0, device=dev)
    ops.rgbnet_bwd(params, feat, acts, rgb, gr, count, cap, scratch, pgrad, fgrad, ctx)
    torch.cuda.synchronize()
    return dict(out=rgb, acts=acts, scratch=scratch, feat_grad=fgrad, pgrad=pgrad)


def _compare(a, b, exact_pgrad, what):
    for k in a:
        if k != 'pgrad':
            _same(a[k], b[k], f'{what}: {k}')
    _atomic_close(a['pgrad'], b['pgrad'], f'{what}: parameter gradients')
    if exact_pgrad:
        _same(a['pgrad'], b['pgrad'], f'{what}: parameter gradients (at most two work-groups)')


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('M', SIZES)
def test_packed_prologue_is_bit_identical(M, scale):
    """Forward and data-gradient kernels of both nets through a context with mlp_pack = 1 (pack recorded: the kernels read it)
    and one with mlp_pack = 0 (today's prologues): out / rgb, all of acts, all of scratch (Ybar), pts_grad / feat_grad are equal
    bit for bit; the pack buffer's fences survive."""
    from poseprobe_amd import ops
    warp, rgbp = _params(scale)
    on, off = ops.Context(mlp_pack=1), ops.Context(mlp_pack=0)
    n = ops.mlp_pack_workspace()
    arena, pack = _fenced(n)
    ops.mlp_pack(warp, rgbp, pack, on)
    ops.mlp_pack(warp, rgbp, pack, off)                      # option off: records nothing, launches nothing
    _compare(_run_warp(warp, M, on), _run_warp(warp, M, off), M <= 32, f'warp net, M = {M}, weights x {scale}')
    _compare(_run_rgb(rgbp, M, on), _run_rgb(rgbp, M, off), M <= 128, f'rgbnet, M = {M}, weights x {scale}')
    _intact(arena, n, 'weight pack')
    ops.mlp_pack_invalidate(on)


def test_pack_is_read_only_for_the_buffer_it_was_made_from():
    """After pp_mlp_pack for one parameter buffer, a call with ANOTHER buffer and the same context gives that buffer's own,
    unpacked results - also when only one net was packed, and after pp_mlp_pack_invalidate."""
    from poseprobe_amd import ops
    M = 1000
    warp_a, rgb_a = _params(0.09)
    warp_b, rgb_b = (t * 1.7 for t in _params(0.09))
    on, off = ops.Context(mlp_pack=1), ops.Context(mlp_pack=0)
    pack = torch.empty(ops.mlp_pack_workspace(), device='cuda')
    ref_w, ref_r = _run_warp(warp_b, M, off), _run_rgb(rgb_b, M, off)
    assert not torch.equal(ref_w['out'], _run_warp(warp_a, M, off)['out'])          # the two buffers do give different results
    ops.mlp_pack(warp_a, rgb_a, pack, on)
    _compare(_run_warp(warp_b, M, on), ref_w, False, 'warp net, other buffer')
    _compare(_run_rgb(rgb_b, M, on), ref_r, False, 'rgbnet, other buffer')
    ops.mlp_pack(warp_b, None, pack, on)                     # rgbnet not packed: its calls derive everything themselves
    _compare(_run_warp(warp_b, M, on), ref_w, False, 'warp net, packed alone')
    _compare(_run_rgb(rgb_b, M, on), ref_r, False, 'rgbnet, not packed')
    ops.mlp_pack(warp_a, rgb_a, pack, on)
    ops.mlp_pack_invalidate(on)
    pack.fill_(float('nan'))                                 # nobody may read it now
    _compare(_run_warp(warp_a, M, on), _run_warp(warp_a, M, off), False, 'warp net, invalidated')
    _compare(_run_rgb(rgb_a, M, on), _run_rgb(rgb_a, M, off), False, 'rgbnet, invalidated')


def test_option_is_listed_and_defaults_to_on():
    from poseprobe_amd import _lib
    assert 'mlp_pack' in _lib.OPTION_NAMES and _lib.library_default('mlp_pack') == 1


def _engine(options):
    from oracle import voxurf_oracle as O
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    G, H, W, N, V = 16, 24, 24, 96, 3
    rs = syn.range_shape()
    views = syn.make_views(V, H, W)
    scene = O.Scene(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, output_range=float(rs.max()), rect_size=rs.tolist())
    P = O.init_params(scene, seed=2)
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(rs.max()))
    eng = TrainEngine(cfg, V, H, W, N, device='cuda:0', deterministic_scatter=True, options=options)
    eng.set_views(views['images'], views['masks'], views['Ks'], views['w2c'])
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'],
                              se3=torch.tensor(syn.se3_perturbation(V)))
    return eng, (V * H * W, N)


def test_engine_repacks_after_an_in_place_parameter_write():
    """A train step, then flat.data overwritten IN PLACE from outside (what bench.py's restore_training_state does: the engine
    cannot see it), then the next step: the engine that packs gives the outputs of an engine with mlp_pack = 0 given the same
    writes.  Both start the second step from one state (the first step's float atomics leave the two apart in the last bit)."""
    from poseprobe_amd import synthetic as syn
    a, (npix, N) = _engine({'mlp_pack': 1})
    b, _ = _engine({'mlp_pack': 0})
    assert a.ctx.get('mlp_pack') == 1 and b.ctx.get('mlp_pack') == 0
    dev = 'cuda:0'
    idx, jit = syn.step_randomness(npix, N, seed=1)
    for e in (a, b):
        e.train_step(torch.tensor(idx, dtype=torch.int32, device=dev), torch.tensor(jit, device=dev), 10)
    g = torch.Generator().manual_seed(11)
    new = (a.flat.data.cpu() * (1.0 + 0.2 * torch.randn(a.flat.data.numel(), generator=g))).to(dev)
    first = a.ws.rgb.clone()
    for e in (a, b):
        e.flat.data.copy_(new)                               # in place: same pointer, new values
        if e is b:
            b.k0_cl.copy_(a.k0_cl); b.se3.copy_(a.se3)
        e.zero_grads()
    for e in (a, b):
        e.render_and_grads(torch.tensor(idx, dtype=torch.int32, device=dev), torch.tensor(jit, device=dev), 11)
    torch.cuda.synchronize()
    M = int(a.ws.count.item())
    assert M == int(b.ws.count.item()) and M > 0
    assert not torch.equal(first[:M], a.ws.rgb[:M])          # the write did change the colours
    for name in ('warp_out', 'rgb', 'g_feat', 'g_warp_out'):
        _same(getattr(a.ws, name)[:M], getattr(b.ws, name)[:M], f'engine step after an in-place write: {name}')
    _same(a.ws.rgb_marched, b.ws.rgb_marched, 'engine step after an in-place write: rgb_marched')
    _same(a.ws.scratch[:4 * M * 128], b.ws.scratch[:4 * M * 128], 'engine step after an in-place write: Ybar3 of the warp net')
