"""The data-gradient kernels of the two MLPs (pp_rgbnet_bwd, pp_warp_bwd, split-precision form) where a work-group walks SEVERAL
tiles.  From its second tile on a work-group takes the `more` path: the next tile's rows and gates are in flight while the tile
before it is still computing, in buffers that tile frees stage by stage, behind counted waits ("loads that span
stages"), and the next tile's output-layer backward runs at the end of the tile before it.  A work-group that owns ONE tile never
takes that path, so

- per-row outputs of a run with one tile per work-group and of runs with option mlp_wgs = 1 / 2 must be equal bit for bit
  (a hazard of the pipeline - a buffer overwritten too early, a wait that covers too little - shows as a difference);
- at the same shapes every output, per row and the thin-layer sums W3bar / b3bar / W4bar / b4bar, is checked against a float64
  evaluation of the same network: the split-precision kernels' error must not exceed the fp32-instruction kernels'
  (mlp_split = 0) on the same inputs by more than a quarter - the bound of tests/test_hip_mlp.py;
- deterministic mode stays bit-reproducible from run to run.

Shapes: one row, one short of a tile, a ragged last tile behind three full ones, five full tiles (rgbnet: 64-row tiles; warp net:
16 samples = 64 rows per tile).  The library raises option mlp_wgs to at least 16 work-groups (the weight-gradient chains share
them out over the layers), so at those four shapes mlp_wgs = 1 / 2 still leaves every work-group with one tile; a fifth shape of
35 full tiles and a ragged one gives each of the 16 work-groups two or three tiles, which is where the `more` path runs.

The error of a quantity is pooled over the five shapes (see _pooled).  The output layer's backward (Ybar3, rgbnet's Ybar2) is
the case these checks found: as a split-precision product with K = 4 / 3 it had twice the fp32 instructions' error (9.6e-08
against 4.6e-08: operands with 22 significant bits and no 128-term sum to hide them under); it is an fp32 MFMA product now."""
import functools
import hashlib

import pytest
import torch

from tests.helpers import load, params_from_npz
from tests.test_hip_mlp import OUT_RANGE, _pack, _rgb_params, _warp_params

pytestmark = pytest.mark.gpu

RGB_ROWS = (1, 63, 64 * 3 + 5, 64 * 5, 64 * 35 + 5)
WARP_SAMPLES = (1, 15, 16 * 3 + 7, 16 * 5, 16 * 35 + 7)
SCALES = ((1.0, 1.0), (1e-3, 1e-6))         # (weights, incoming gradients), as tests/test_hip_mlp.py


def _dev_params(P):
    params = torch.zeros(P.numel() + 60, device='cuda')
    params[:P.numel()] = P.to('cuda')
    return params


def _rgb_inputs(R, wscale=1.0, gscale=1.0):
    from poseprobe_amd.engine import pack_rgbnet
    g = torch.Generator().manual_seed(100 + R)
    layers = [(W * (wscale if i < 3 else 1.0), b * wscale) for i, (W, b) in enumerate(_rgb_params(5))]
    feat = torch.zeros(R, 64)
    feat[:, :57] = torch.randn(R, 57, generator=g)
    gr = torch.randn(R, 3, generator=g) * gscale * torch.exp(torch.randn(R, 1, generator=g) * 2)
    return layers, pack_rgbnet(layers), feat, gr


def _rgb_run(R, P, feat, gr, cx, data_only):
    """-> (ybar [3][R][128], feat_grad [R][64], params_grad) of one forward + backward with context cx."""
    from poseprobe_amd import ops
    dev = 'cuda'
    params = _dev_params(P)
    count = torch.tensor([R], dtype=torch.int32, device=dev)
    acts = torch.zeros(3 * R * 128, device=dev)
    rgb = torch.zeros(R, 3, device=dev)
    ops.rgbnet_fwd(params, feat.to(dev), count, R, acts, rgb, cx)
    scratch = torch.zeros(3 * R * 128 + 49152, device=dev)
    pgrad = torch.zeros_like(params)
    fgrad = torch.zeros(R, 64, device=dev)
    if data_only:
        ops.rgbnet_bwd_data(params, acts, rgb, gr.to(dev), count, R, scratch, pgrad, fgrad, cx)
    else:
        ops.rgbnet_bwd(params, feat.to(dev), acts, rgb, gr.to(dev), count, R, scratch, pgrad, fgrad, cx)
    torch.cuda.synchronize()
    return scratch[:3 * R * 128].view(3, R, 128).clone(), fgrad, pgrad[:P.numel()].clone()


def _warp_inputs(M, wscale=1.0, gscale=1.0):
    g = torch.Generator().manual_seed(200 + M)
    layers = [(W * (wscale if 0 < i < 4 else 1.0), b * wscale) for i, (W, b) in enumerate(_warp_params(3))]
    pts = torch.randn(M, 3, generator=g) * 0.5
    og = torch.randn(M, 16, generator=g) * gscale * torch.exp(torch.randn(M, 1, generator=g) * 2)
    return layers, _pack(layers), pts, og


def _warp_run(M, P, pts, og, cx, lean, data_only):
    """-> (ybar [3][4M][128], pts_grad [M][3], params_grad); lean: inside a lean scope of the buffers (Ybar3 is then not stored:
    plane 0 starts with the tile-wise output gradients instead)."""
    from poseprobe_amd import ops
    dev = 'cuda'
    params = _dev_params(P)
    count = torch.tensor([M], dtype=torch.int32, device=dev)
    acts = torch.zeros(4 * M * 4 * 128, device=dev)
    out = torch.zeros(M, 16, device=dev)
    scratch = torch.zeros(3 * M * 4 * 128 + 49152, device=dev)
    pgrad = torch.zeros_like(params)
    ptsg = torch.zeros(M, 3, device=dev)
    if lean:
        ops.warp_lean_begin(acts, scratch, params, cx)
    try:
        ops.warp_fwd(params, pts.to(dev), count, M, OUT_RANGE, acts, out, cx)
        if data_only:
            ops.warp_bwd_data(params, pts.to(dev), acts, og.to(dev), count, M, OUT_RANGE, scratch, pgrad, ptsg, cx)
        else:
            ops.warp_bwd(params, pts.to(dev), acts, og.to(dev), count, M, OUT_RANGE, scratch, pgrad, ptsg, cx)
        torch.cuda.synchronize()
    finally:
        if lean:
            ops.warp_lean_end(cx)
    return scratch[:3 * M * 4 * 128].view(3, 4 * M, 128).clone(), ptsg, pgrad[:P.numel()].clone()


# ------------------------------------------------------------------------------------------------ hazards
@pytest.mark.parametrize('R', RGB_ROWS)
def test_rgbnet_rows_do_not_depend_on_how_many_tiles_a_work_group_walks(R):
    from poseprobe_amd import ops
    _, P, feat, gr = _rgb_inputs(R)
    y1, f1, _ = _rgb_run(R, P, feat, gr, ops.Context(), data_only=True)          # one tile per work-group
    assert bool((y1 != 0).any()) and bool((f1 != 0).any())
    for wgs in (1, 2):
        y, f, _ = _rgb_run(R, P, feat, gr, ops.Context(mlp_wgs=wgs), data_only=True)
        assert torch.equal(y, y1), f'mlp_wgs = {wgs}: ybar differs in {int((y != y1).sum())} entries'
        assert torch.equal(f, f1), f'mlp_wgs = {wgs}: feat_grad differs in {int((f != f1).sum())} entries'


@pytest.mark.parametrize('lean', [True, False], ids=['lean', 'full'])
@pytest.mark.parametrize('M', WARP_SAMPLES)
def test_warp_rows_do_not_depend_on_how_many_tiles_a_work_group_walks(M, lean):
    from poseprobe_amd import ops
    _, P, pts, og = _warp_inputs(M)
    y1, p1, _ = _warp_run(M, P, pts, og, ops.Context(), lean, data_only=True)
    assert bool((y1 != 0).any()) and bool((p1 != 0).any())
    for wgs in (1, 2):
        y, p, _ = _warp_run(M, P, pts, og, ops.Context(mlp_wgs=wgs), lean, data_only=True)
        assert torch.equal(y, y1), f'mlp_wgs = {wgs}: ybar differs in {int((y != y1).sum())} entries'
        assert torch.equal(p, p1), f'mlp_wgs = {wgs}: pts_grad differs in {int((p != p1).sum())} entries'


# ------------------------------------------------------------------------------------------------ values
# The bound compares two rounding errors, and an RMS over n roundings is itself known to 1 / sqrt(2 n) only: the ratio of two of
# them over the 64 open entries of ONE row scatters by 12 %, over the 3 entries of b3bar by more than half (the order of its
# atomic sums changes from run to run on top), and a bound of a quarter would then fail or pass by chance.  So a quantity's error
# is pooled over the five shapes entry by entry: every entry's squared error over its own tensor's mean square of the reference,
# the mean over ALL entries of the five shapes, the root; the sums of the output layer (W3bar with b3bar, W4bar with b4bar) are
# pooled the same way, each part over its own mean square.  (Not a mean of per-shape figures: pts_grad has 3 entries at the
# one-sample shape and 45 at the next, and a fifth of the weight each would put a figure known to 40 % into the pool - the pooled
# ratio would scatter by a sixth; entry by entry it rests on 2 154 entries, 2 %.)  Nothing a wrong value would show is lost: one
# wrong entry at any shape is an error of order 1 x sqrt(1 / 360 000) = 2e-3 for a hidden layer's rows, more for everything
# smaller, in a figure of 2e-7.
def _msq(a, ref):
    """(sum of squared errors over the mean square of the reference, entries)"""
    a, ref = a.detach().double().cpu(), ref.detach().double()
    return float(((a - ref) ** 2).sum() / max(float((ref ** 2).mean()), 1e-300)), ref.numel()


def _pooled(per_shape):
    """per_shape: [{name: [(sse, n), ...]}, ...] -> {name: pooled relative RMS error}"""
    out = {}
    for name in per_shape[0]:
        parts = [p for sh in per_shape for p in sh[name]]
        out[name] = (sum(s for s, _ in parts) / sum(n for _, n in parts)) ** 0.5
    return out


def _assert_bound(errs, name, what):
    from poseprobe_amd import _lib
    a, b = errs[0][name], errs[_lib.get_option('mlp_split')][name]
    print(f'{what}: {name}: fp32 {a:.3e}, split {b:.3e}')
    assert b <= 1.25 * a + 1e-12, f'{what}: {name}: fp32 {a:.3e}, split {b:.3e}'


@functools.lru_cache(maxsize=None)
def _rgb_errors(wscale, gscale):
    """-> {mode: {quantity: pooled error}}, computed once for all tests of this pair of scales."""
    from poseprobe_amd import ops, _lib
    from poseprobe_amd.engine import unpack_rgbnet
    default = _lib.get_option('mlp_split')
    shapes = {0: [], default: []}
    for R in RGB_ROWS:
        layers, P, feat, gr = _rgb_inputs(R, wscale, gscale)
        lay = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in layers]
        x = feat[:, :57].double().requires_grad_(True)
        h, pre = x, []
        for li, (W, b) in enumerate(lay):
            z = h @ W.T + b
            if li < 3:
                z.retain_grad()
                pre.append(z)
            h = torch.relu(z) if li < 3 else torch.sigmoid(z)
        (h * gr.double()).sum().backward()
        for mode in (0, default):
            y, f, pg = _rgb_run(R, P, feat, gr, ops.Context(mlp_split=mode, mlp_wgs=2), data_only=False)
            (gW3, gb3) = unpack_rgbnet(pg)[3]
            shapes[mode].append({'Ybar2': [_msq(y[0], pre[2].grad)], 'Ybar1': [_msq(y[1], pre[1].grad)],
                                 'Ybar0': [_msq(y[2], pre[0].grad)], 'feat_grad': [_msq(f[:, :57], x.grad)],
                                 'W3bar+b3bar': [_msq(gW3, lay[3][0].grad), _msq(gb3, lay[3][1].grad)]})
    return {mode: _pooled(v) for mode, v in shapes.items()}


@pytest.mark.parametrize('wscale,gscale', SCALES)
@pytest.mark.parametrize('name', ['Ybar2', 'Ybar1', 'Ybar0', 'feat_grad', 'W3bar+b3bar'])
def test_rgbnet_backward_is_as_accurate_as_the_fp32_instructions(name, wscale, gscale):
    _assert_bound(_rgb_errors(wscale, gscale), name, f'rgbnet, weights x {wscale}, gradients x {gscale}')


def _warp_ref64(layers, pts):
    """tests/test_hip_mlp.py::_warp_ref, keeping the hidden layers' pre-activations (their gradients are Ybar1 .. Ybar3)."""
    (W0, b0) = layers[0]
    y0 = pts @ W0.T + b0
    m = (y0 > 0).to(y0.dtype)
    X = torch.stack([y0 * m, m * W0[:, 0], m * W0[:, 1], m * W0[:, 2]], dim=1)
    pre = []
    for W, b in layers[1:4]:
        Y = X @ W.T
        Y = torch.cat([Y[:, :1] + b, Y[:, 1:]], dim=1)
        Y.retain_grad()
        pre.append(Y)
        X = Y * (Y[:, :1] > 0).to(Y.dtype)
    W4, b4 = layers[4]
    out = X @ W4.T
    out = torch.cat([out[:, :1] + b4, out[:, 1:]], dim=1)
    return out * OUT_RANGE, pre


@functools.lru_cache(maxsize=None)
def _warp_errors(wscale, gscale, lean):
    from poseprobe_amd import ops, _lib
    default = _lib.get_option('mlp_split')
    shapes = {0: [], default: []}
    for M in WARP_SAMPLES:
        layers, P, pts, og = _warp_inputs(M, wscale, gscale)
        lay = [(W.double().requires_grad_(True), b.double().requires_grad_(True)) for W, b in layers]
        p = pts.double().requires_grad_(True)
        ref, pre = _warp_ref64(lay, p)
        (ref.reshape(M, 16) * og.double()).sum().backward()
        o4 = P.numel() - 4 * 128 - 4
        for mode in (0, default):
            # (the fp32-instruction kernels have no lean form: their run is the full one in both scopes)
            y, pg_pts, pg = _warp_run(M, P, pts, og, ops.Context(mlp_split=mode, mlp_wgs=2), lean and mode != 0, data_only=False)
            e = {'Ybar2': [_msq(y[1], pre[1].grad.reshape(4 * M, 128))], 'Ybar1': [_msq(y[2], pre[0].grad.reshape(4 * M, 128))],
                 'pts_grad': [_msq(pg_pts, p.grad)],
                 'W4bar+b4bar': [_msq(pg[o4:o4 + 512].view(4, 128), lay[4][0].grad), _msq(pg[o4 + 512:o4 + 516], lay[4][1].grad)]}
            if not lean:
                e['Ybar3'] = [_msq(y[0], pre[2].grad.reshape(4 * M, 128))]
            shapes[mode].append(e)
    return {mode: _pooled(v) for mode, v in shapes.items()}


# (Ybar3 is not stored in the lean scope: the weight-gradient kernel rebuilds it, tests/test_hip_warp_lean.py)
WARP_CASES = [pytest.param(name, lean, id=f'{name}-{"lean" if lean else "full"}') for lean in (True, False)
              for name in ('Ybar3', 'Ybar2', 'Ybar1', 'pts_grad', 'W4bar+b4bar') if not (lean and name == 'Ybar3')]


@pytest.mark.parametrize('wscale,gscale', SCALES)
@pytest.mark.parametrize('name,lean', WARP_CASES)
def test_warp_backward_is_as_accurate_as_the_fp32_instructions(name, lean, wscale, gscale):
    _assert_bound(_warp_errors(wscale, gscale, lean), name,
                  f'warp, weights x {wscale}, gradients x {gscale}, {"lean" if lean else "full"} scope')


# ------------------------------------------------------------------------------------------------ deterministic mode
def _deterministic_hash(n_steps):
    from poseprobe_amd import synthetic as syn
    from poseprobe_amd.engine import SceneConfig, TrainEngine
    d = load('forward_g24_s10.npz')
    G, H, W, N = int(d['G']), int(d['H']), int(d['W']), 256
    assert G == 24
    cfg = SceneConfig(syn.XYZ_MIN, syn.XYZ_MAX, G ** 3, out_range=float(syn.range_shape().max()))
    eng = TrainEngine(cfg, 3, H, W, N, pose_iters=1000, deterministic=True)
    eng.set_views(d['images'], d['masks'], d['Ks'], d['w2c_init'])
    P = params_from_npz(d)
    eng.load_reference_params(P['k0'], P['sdf'], P['sdf_alpha'], P['sdf_beta'], P['rgbnet'], P['warp'], se3=torch.tensor(d['se3']))
    eng.zero_grads()
    V = d['images'].shape[0]
    first = eng.flat.data.detach().clone()
    for s in range(n_steps):
        idx, jit = syn.step_randomness(V * H * W, N, seed=40 + s)
        eng.train_step(torch.tensor(idx, dtype=torch.int32, device='cuda'), torch.tensor(jit, device='cuda'), 10 + s)
    torch.cuda.synchronize()
    assert bool((eng.flat.data != first).any())
    return hashlib.sha256(eng.flat.data.detach().cpu().numpy().tobytes()).hexdigest()


def test_deterministic_mode_gives_the_same_bits_twice():
    """Two three-step runs of TrainEngine(deterministic=True), 24^3 grid, 256 rays: equal hashes of flat.data."""
    assert _deterministic_hash(3) == _deterministic_hash(3)
