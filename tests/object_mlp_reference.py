"""The object branch's two MLP chains (csrc/pp_mlp.hip: pp_warp_fwd / pp_warp_bwd, pp_rgbnet_fwd / pp_rgbnet_bwd) stage by stage: the
layouts of the blocks the kernels read and leave behind, restated from include/poseprobe_hip.h and csrc/pp_mlp_fused.h, and one
float64 / float32 reference per stage (TEST INFRASTRUCTURE ONLY).

A pass keeps its intermediates: the warp net's `acts` is [4][cap * 4][128] = X0 .. X3 in 4-row form (row 4 s + r of sample s, r = 0
the primal row, r = 1 .. 3 the tangents d / d p_i), its `scratch` is [3][cap * 4][128] = Ybar3, Ybar2, Ybar1; rgbnet's `acts` is
[3][cap][128] = H0 .. H2 and its `scratch` [3][cap][128] = Ybar2, Ybar1, Ybar0.  Each stage is therefore compared with an evaluation
of THAT STAGE ALONE on the kernel's own stored inputs, and every ReLU gate of a reference that multiplies a tangent row or a gradient
is (stored primal activation > 0): no state can differ between kernel and reference, no row needs excusing, and helpers.check
applies to every entry.  (A primal forward row is relu of the reference's own pre-activation: ReLU is continuous, nothing can flip.)

Three images of the warp net's blocks (`form`):
  'full'     everything above is stored;
  'lean'     inside pp_warp_lean_begin: slot 0 of `acts` holds the primal rows only, floats [0, 16 M) of slot 0 of `scratch` hold
             out_range * out_grad at 16 s + 4 r + j, the rest of both slots is untouched; the references REBUILD the tangent rows of
             X0 (exactly: gate0 W0[:, i]) and Ybar3 (float64, from the stored image) for the stages that consume them;
  'layered'  option mlp_fused = 0: the layer-by-layer backward ping-pongs between slots 0 and 1, so what is left is Ybar1 in slot 0 and
             Ybar0 in slot 1 (rgbnet: Ybar0 in slot 0, Ybar1 in slot 1); the stages whose stored input was overwritten (Ybar2, Ybar1 as
             products, W3bar, W2bar and their bias sums; rgbnet: Ybar2, Ybar1, W2bar, b2bar) have nothing to be compared on.

Every stage function returns (ref64, ref32, scale): the expression in float64, the same expression in torch float32 (a blocked
library product: another association than the kernels'), and the summed magnitudes of the terms behind an entry - for a product
sum_k |a_k| |b_k| (+ |bias|), for a weight gradient sum_rows |Ybar| |X|.  Where an operand was itself rebuilt or is unstored (Ybar3
in lean form, Ybar0 of the warp net, which its kernel keeps in LDS), its own scale stands in for its magnitude: the scale carries both
products.  rgb = sigmoid(s), s = H2 W3^T + b3, has the scene test's reasoned scale |value| + sigmoid'(s) (sum |h| |W3| + |b3|).
tests/test_object_mlp_reference.py ties the chained float64 stages to oracle.voxurf_oracle.warp_mlp / rgbnet_mlp with autograd and to
tests/analytic_model.warp_forward / warp_backward (1e-12) and measures what float32 in a third association (`emulate32_*`) needs.
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests.scene_ray_reference import ulps_needed  # noqa: F401  (re-exported: the tests print what each stage needs)

F64, F32 = torch.float64, torch.float32
SENT = 0x7FC0DEAD                                           # a quiet-NaN payload no kernel produces
TAIL = 49152                                                # floats behind the Ybar slots of either `scratch` (transposed weights)
HALF_ROWS = 32                                              # rows that share one operand scale in the split-precision kernels

# ------------------------------------------------------------------------------------------------------------------- layouts
# WPF_* of csrc/pp_mlp_fused.h: W0[128 x 3] b0 | W1 .. W3[128 x 128] b | W4[4 x 128] b4
WARP_SHAPES = ((128, 3), (128, 128), (128, 128), (128, 128), (4, 128))
# RGF_*: W0[128 x 64] b0 | W1[128 x 128] b1 | W2[128 x 128] b2 | W3[3 x 128] b3 (W0: the [128, 57] weight zero-padded to 64 columns)
RGB_SHAPES = ((128, 64), (128, 128), (128, 128), (3, 128))
RGB_IN = 57
WARP_PARAMS = sum(o * k + o for o, k in WARP_SHAPES)
RGB_PARAMS = sum(o * k + o for o, k in RGB_SHAPES)


def _param_views(flat, shapes):
    P, o = {}, 0
    for l, (n, k) in enumerate(shapes):
        P[f'W{l}'] = flat[o:o + n * k].view(n, k)
        o += n * k
        P[f'b{l}'] = flat[o:o + n]
        o += n
    return P


def warp_param_views(flat):
    """{W0 [128, 3], b0, W1 .. W3 [128, 128], b1 .. b3, W4 [4, 128], b4} of a packed warp parameter (or gradient) block."""
    return _param_views(flat, WARP_SHAPES)


def rgb_param_views(flat):
    return _param_views(flat, RGB_SHAPES)


def workspace_floats(cap):
    """{'rgbnet': (acts, scratch), 'warp': (acts, scratch)} in floats: what ops.mlp_workspaces(cap) must return."""
    return {'rgbnet': (3 * cap * 128, 3 * cap * 128 + TAIL), 'warp': (4 * cap * 4 * 128, 3 * cap * 4 * 128 + TAIL)}


def warp_acts_view(acts, cap):
    return acts[:4 * cap * 4 * 128].view(4, cap * 4, 128)     # [layer][4 s + r][feature]


def warp_scratch_view(scratch, cap):
    return scratch[:3 * cap * 4 * 128].view(3, cap * 4, 128)


def rgb_acts_view(acts, cap):
    return acts[:3 * cap * 128].view(3, cap, 128)


def rgb_scratch_view(scratch, cap):
    return scratch[:3 * cap * 128].view(3, cap, 128)


def bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------- stage references
def _t(x, dt):
    return torch.as_tensor(x).to(dt)


def _three(expr, *xs, gate=None, post=None, mags=None):
    """(expr in float64, expr in float32, expr on the magnitudes); mags: {index: scale that stands in for |xs[index]|}."""
    x64 = [_t(x, F64) for x in xs]
    xa = [x.abs() if not (mags and i in mags) else _t(mags[i], F64) for i, x in enumerate(x64)]
    r64, r32, sc = expr(*x64), expr(*[_t(x, F32) for x in xs]), expr(*xa)
    if post is not None:
        r64, r32 = post(r64), post(r32)
    if gate is not None:
        r64, r32, sc = r64 * gate.to(F64), r32 * gate.to(F32), sc * gate.to(F64)
    return r64, r32, sc


def primal_rows(n_rows, rmul, dev):
    """[n_rows, 1] bool: the rows that carry a bias and a ReLU of their own (rmul = 4: every fourth row; 1: all)."""
    return (torch.arange(n_rows, device=dev) % rmul == 0)[:, None]


def row_gate(act, rmul):
    """[rows, 128] bool: (stored primal activation > 0) of a row's sample, for all rmul rows of the sample."""
    return (torch.as_tensor(act)[::rmul] > 0).repeat_interleave(rmul, 0)


def warp_x0(pts, W0, b0, X0_stored):
    """Layer 0 of the 4-row form -> triple of [4 M, 128]: primal rows relu(W0 p + b0); tangent rows gate0 W0[:, i], which are exact
    (ref64 = ref32 = the value): gate0 from the STORED primal rows."""
    M = pts.shape[0]
    p64, p32, psc = _three(lambda p, W, b: p @ W.T + b, pts, W0, b0, post=torch.relu)
    g = torch.as_tensor(X0_stored)[::4] > 0                                            # [M, 128]
    out = []
    for prim, dt in ((p64, F64), (p32, F32), (psc, F64)):
        tang = torch.where(g[:, None, :], _t(W0, dt).T[None], torch.zeros((), dtype=dt, device=g.device))   # [M, 3, 128]; closed: +0
        full = torch.cat([prim[:, None], tang.abs() if prim is psc else tang], 1)
        out.append(full.reshape(4 * M, 128))
    return tuple(out)


def rebuilt_x0(X0_stored, W0):
    """X0 with its tangent rows rebuilt from the stored primal rows (the lean image): float32, exact."""
    X = torch.as_tensor(X0_stored).clone()
    M = X.shape[0] // 4
    X.view(M, 4, 128)[:, 1:] = torch.where((X[::4] > 0)[:, None, :], torch.as_tensor(W0).to(X.dtype).T[None], torch.zeros((), dtype=X.dtype, device=X.device))
    return X


def hidden(Xprev, W, b, X_stored, rmul):
    """Layer l >= 1: primal rows relu(Xprev W^T + b), tangent rows gate_l (Xprev W^T), gate_l from the stored primal rows of X_l."""
    prim = primal_rows(Xprev.shape[0], rmul, torch.as_tensor(Xprev).device)
    r64, r32, sc = _three(lambda x, W, b: x @ W.T + b * prim.to(x.dtype), Xprev, W, b)
    g = row_gate(X_stored, rmul)
    fin = lambda r: torch.where(prim, torch.relu(r), r * g.to(r.dtype))
    return fin(r64), fin(r32), torch.where(prim, sc, sc * g.to(F64))


def warp_out(X3, W4, b4, out_range):
    """out_range (X3 W4^T + b4 on the primal rows) -> [4 M, 4]; the kernels' out[s][r][j] is this at row 4 s + r, column j."""
    prim = primal_rows(X3.shape[0], 4, torch.as_tensor(X3).device)
    return _three(lambda x, W, b: (x @ W.T + b * prim.to(x.dtype)) * out_range, X3, W4, b4)         # (out_range > 0)


def rgb_out(H2, W3, b3):
    s64, s32, ssc = _three(lambda h, W, b: h @ W.T + b, H2, W3, b3)
    r64, r32 = torch.sigmoid(s64), torch.sigmoid(s32)
    return r64, r32, r64 + r64 * (1 - r64) * ssc


def _gl(g, c):
    return g * c * (1 - c)                                   # d loss / d (pre-sigmoid), on the stored colours c in [0, 1]


def data_grad(Y, W, act, rmul, y_scale=None):
    """gate (Y W): Y [rows, N] the gradient of a layer's pre-activations, W [N, K] its weights, gate = (stored primal `act` > 0)."""
    return _three(lambda Y, W: Y @ W, Y, W, gate=row_gate(act, rmul), mags=None if y_scale is None else {0: y_scale})


def grad_w(Y, X, y_scale=None):
    return _three(lambda Y, X: Y.T @ X, Y, X, mags=None if y_scale is None else {0: y_scale})


def grad_b(Y, rmul, y_scale=None):
    """Column sums over the primal rows."""
    return _three(lambda Y: Y[::rmul].sum(0), Y, mags=None if y_scale is None else {0: y_scale})


def half_scale(scale, rows=HALF_ROWS):
    """The scale of the planted case 'range' for a row-wise stage: the largest scale of the entry's half (`rows` consecutive rows,
    all columns) - the kernels' operand scale of a half comes from the half's largest magnitude whatever its column."""
    R, C = scale.shape
    Rp = (R + rows - 1) // rows * rows
    s = torch.zeros(Rp, C, dtype=scale.dtype, device=scale.device)
    s[:R] = scale
    return s.view(-1, rows, C).amax((1, 2), keepdim=True).expand(-1, rows, C).reshape(Rp, C)[:R]


SHARED_FLOOR = 2.0 ** -18


def shared_scale_floor(Y, X, y_scale=None):
    """The planted case 'range' for a weight gradient of the split-precision chain: k_wgrad_chain_s converts both operands with ONE
    power of two per operand for a work-group's whole row range and an absolute floor of 2^-40 of the largest magnitude that scale
    holds (a factor 4 of headroom: 2^-38), "which is what a sum needs" (pp_mlp_split.hip, weight gradients).  An entry's error from
    the floor is at most sum_r (2^-38 max|Y| |X[r][k]| + |Y[r][n]| 2^-38 max|X|); as a scale under 8 eps32 = 2^-20 that is
    2^-18 (max|Y| sum_r |X[r][k]| + max|X| sum_r |Y[r][n]|), added to the entry's own."""
    Ya = _t(Y, F64).abs() if y_scale is None else _t(y_scale, F64)
    Xa = _t(X, F64).abs()
    if Ya.numel() == 0:
        return 0.0
    return SHARED_FLOOR * (Ya.max() * Xa.sum(0)[None, :] + Xa.max() * Ya.sum(0)[:, None])


# -------------------------------------------------------------------------------------------------------------- a finished pass
def make_warp_run(form, flat, grad, acts, scratch, out, pts, out_grad, pts_grad, prefill, M, cap, out_range):
    """Everything a forward + backward pass of the warp net read and left behind (tensors of one device); M = min(count, cap)."""
    assert form in ('full', 'lean', 'layered')
    return SimpleNamespace(form=form, M=M, cap=cap, out_range=float(np.float32(out_range)), P=warp_param_views(flat), G=warp_param_views(grad),
                           X=warp_acts_view(acts, cap), S=warp_scratch_view(scratch, cap), out=out, pts=pts, out_grad=out_grad,
                           pts_grad=pts_grad, prefill=prefill)


def make_rgb_run(form, flat, grad, acts, scratch, rgb, feat, rgb_grad, feat_grad, M, cap):
    assert form in ('full', 'layered')
    return SimpleNamespace(form=form, M=M, cap=cap, P=rgb_param_views(flat), G=rgb_param_views(grad), H=rgb_acts_view(acts, cap),
                           S=rgb_scratch_view(scratch, cap), rgb=rgb, feat=feat, rgb_grad=rgb_grad, feat_grad=feat_grad)


def _sample_rows(samples, dev):
    return (4 * samples[:, None] + torch.arange(4, device=dev)[None]).reshape(-1)


def _warp_x(run, rows):
    """X0 .. X3 on the rows `rows`, X0 with rebuilt tangents in lean form."""
    X = [run.X[l][rows] for l in range(4)]
    if run.form == 'lean':
        X[0] = rebuilt_x0(X[0], run.P['W0'])
    return X


def warp_forward_stages(run, samples=None):
    """-> (name, the pass's value, (ref64, ref32, scale)) per forward stage; samples: a subset (the stages are row-independent)."""
    P, dev = run.P, run.out.device
    s = torch.arange(run.M, device=dev) if samples is None else samples
    rows = _sample_rows(s, dev)
    stored0 = run.X[0][rows]
    t0 = warp_x0(run.pts[s], P['W0'], P['b0'], stored0)
    if run.form == 'lean':                                   # only the primal rows were written
        yield 'X0', stored0[::4], tuple(t[::4] for t in t0)
    else:
        yield 'X0', stored0, t0
    X = _warp_x(run, rows)
    for l in (1, 2, 3):
        yield f'X{l}', X[l], hidden(X[l - 1], P[f'W{l}'], P[f'b{l}'], X[l], 4)
    yield 'out', run.out[s].reshape(-1, 4), warp_out(X[3], P['W4'], P['b4'], run.out_range)


def _warp_g(run, s):
    """out_range * out_grad as [4 M', 4] (row 4 s + r, column j): float32, the product the kernels form first."""
    return (run.out_grad[s] * torch.tensor(run.out_range, dtype=F32, device=run.out_grad.device)).reshape(-1, 4)


def _warp_ybar(run, rows, s, X):
    """{l: (Ybar_l on `rows`, scale that stands in for its magnitude or None, stored?)} for l = 3, 2, 1, 0 as far as the form has them."""
    P, Y = run.P, {}
    if run.form == 'full':
        for l in (3, 2, 1):
            Y[l] = (run.S[3 - l][rows], None, True)
    elif run.form == 'lean':
        r64, _, sc = data_grad(run.S[0].reshape(-1)[:16 * run.M].view(-1, 4)[rows], P['W4'], X[3], 4)
        Y[3] = (r64, sc, False)                              # rebuilt in float64 from the stored image
        Y[2], Y[1] = (run.S[1][rows], None, True), (run.S[2][rows], None, True)
    else:
        Y[1] = (run.S[0][rows], None, True)
    y1, sc1, _ = Y[1]
    r64, _, sc = data_grad(y1, P['W1'], X[0], 4, sc1)
    Y[0] = (run.S[1][rows], None, True) if run.form == 'layered' else (r64, sc, False)
    return Y


def warp_data_gradient_stages(run, samples=None):
    """The row-independent backward stages: (the lean image,) Ybar3, Ybar2, Ybar1, (Ybar0 where it is stored,) pts_grad."""
    P, dev = run.P, run.out.device
    s = torch.arange(run.M, device=dev) if samples is None else samples
    rows = _sample_rows(s, dev)
    X = _warp_x(run, rows)
    Y = _warp_ybar(run, rows, s, X)
    g = _warp_g(run, s)
    if run.form == 'full':
        yield 'Ybar3', Y[3][0], data_grad(g, P['W4'], X[3], 4)
    if run.form != 'layered':
        yield 'Ybar2', Y[2][0], data_grad(Y[3][0], P['W3'], X[2], 4, Y[3][1])
        yield 'Ybar1', Y[1][0], data_grad(Y[2][0], P['W2'], X[1], 4)
    else:
        yield 'Ybar0', Y[0][0], data_grad(Y[1][0], P['W1'], X[0], 4)
    y0, sc0, _ = Y[0]
    r64, r32, sc = _three(lambda y, W: y[::4] @ W, y0, P['W0'], mags=None if sc0 is None else {0: sc0})
    pre = run.prefill[s]
    yield 'pts_grad', run.pts_grad[s], (r64 + pre.to(F64), r32 + pre, sc + pre.abs().to(F64))


def warp_weight_gradient_stages(run, shared_range=False):
    """Sums over all rows: W4bar, b4bar, the hidden layers' products with their bias sums, W0bar, b0bar.  shared_range: the hidden
    layers' products carry shared_scale_floor (the planted case 'range' on a split-precision route)."""
    P, G, dev = run.P, run.G, run.out.device
    s = torch.arange(run.M, device=dev)
    rows = _sample_rows(s, dev)
    X = _warp_x(run, rows)
    Y = _warp_ybar(run, rows, s, X)
    g = _warp_g(run, s)
    yield 'W4bar', G['W4'], grad_w(g, X[3])
    yield 'b4bar', G['b4'], grad_b(g, 4)
    for l in (3, 2, 1):
        if l in Y:
            r64, r32, sc = grad_w(Y[l][0], X[l - 1], Y[l][1])
            yield f'W{l}bar', G[f'W{l}'], (r64, r32, sc + shared_scale_floor(Y[l][0], X[l - 1], Y[l][1]) if shared_range else sc)
            yield f'b{l}bar', G[f'b{l}'], grad_b(Y[l][0], 4, Y[l][1])
    y0, sc0, _ = Y[0]
    mags = None if sc0 is None else {0: sc0}
    w0 = lambda y, p: torch.einsum('sn,si->ni', y[::4], p) + y.view(-1, 4, 128)[:, 1:].sum(0).T
    yield 'W0bar', G['W0'], _three(w0, y0, run.pts[s], mags=mags)
    yield 'b0bar', G['b0'], grad_b(y0, 4, sc0)


def warp_stages(run, shared_range=False):
    yield from warp_forward_stages(run)
    yield from warp_data_gradient_stages(run)
    yield from warp_weight_gradient_stages(run, shared_range)


def rgb_forward_stages(run, rows=None):
    P = run.P
    r = torch.arange(run.M, device=run.rgb.device) if rows is None else rows
    H = [run.H[l][r] for l in range(3)]
    x = run.feat[r]
    for l in range(3):
        yield f'H{l}', H[l], hidden(x, P[f'W{l}'], P[f'b{l}'], H[l], 1)
        x = H[l]
    yield 'rgb', run.rgb[r], rgb_out(H[2], P['W3'], P['b3'])


def _rgb_ybar(run, r):
    """{l: Ybar_l on the rows r} as far as the form has them (slots: full 2, 1, 0; layered: Ybar0 in slot 0, Ybar1 in slot 1)."""
    if run.form == 'full':
        return {2: run.S[0][r], 1: run.S[1][r], 0: run.S[2][r]}
    return {0: run.S[0][r], 1: run.S[1][r]}


def rgb_data_gradient_stages(run, rows=None):
    P = run.P
    r = torch.arange(run.M, device=run.rgb.device) if rows is None else rows
    H, Y = [run.H[l][r] for l in range(3)], _rgb_ybar(run, r)
    if 2 in Y:
        yield 'Ybar2', Y[2], _three(lambda g, c, W: _gl(g, c) @ W, run.rgb_grad[r], run.rgb[r], P['W3'], gate=row_gate(H[2], 1))
        yield 'Ybar1', Y[1], data_grad(Y[2], P['W2'], H[1], 1)
    yield 'Ybar0', Y[0], data_grad(Y[1], P['W1'], H[0], 1)
    yield 'feat_grad', run.feat_grad[r], _three(lambda y, W: y @ W, Y[0], P['W0'])


def rgb_weight_gradient_stages(run, shared_range=False):
    G = run.G
    r = torch.arange(run.M, device=run.rgb.device)
    H, Y = [run.H[l][r] for l in range(3)], _rgb_ybar(run, r)
    yield 'W3bar', G['W3'], _three(lambda g, c, h: _gl(g, c).T @ h, run.rgb_grad[r], run.rgb[r], H[2])
    yield 'b3bar', G['b3'], _three(lambda g, c: _gl(g, c).sum(0), run.rgb_grad[r], run.rgb[r])
    for l in (2, 1, 0):
        if l in Y:
            xin = run.feat[r] if l == 0 else H[l - 1]
            r64, r32, sc = grad_w(Y[l], xin)
            yield f'W{l}bar', G[f'W{l}'], (r64, r32, sc + shared_scale_floor(Y[l], xin) if shared_range else sc)
            yield f'b{l}bar', G[f'b{l}'], grad_b(Y[l], 1)


def rgb_stages(run, shared_range=False):
    yield from rgb_forward_stages(run)
    yield from rgb_data_gradient_stages(run)
    yield from rgb_weight_gradient_stages(run, shared_range)


# ---------------------------------------------------------------------------------------------------------------- exact promises
def warp_exact_promises(run):
    """What holds bit for bit: -> list of (what, bool).  Rows past M keep their sentinel (the blocks start as SENT everywhere)."""
    M, cap, dev = run.M, run.cap, run.out.device
    sent = lambda t: bool((bits(t) == SENT).all())
    X, S = run.X, run.S
    out = [('rows of acts past the count keep their sentinel', sent(X[:, 4 * M:])),
           ('rows of out past the count keep their sentinel', sent(run.out[M:])),
           ('rows of pts_grad past the count keep their prefill', torch.equal(bits(run.pts_grad[M:]), bits(run.prefill[M:])))]
    if run.form == 'lean':
        tang = torch.ones(4 * cap, dtype=torch.bool, device=dev)
        tang[0::4] = False
        img = S[0].reshape(-1)
        want = (run.out_grad[:M] * torch.tensor(run.out_range, dtype=F32, device=dev)).reshape(-1)
        out += [('lean: the tangent rows of X0 keep their sentinel', sent(X[0][tang])),
                ('lean: floats [0, 16 M) of scratch slot 0 are the float32 product out_range * out_grad', torch.equal(bits(img[:16 * M]), bits(want))),
                ('lean: the rest of scratch slot 0 keeps its sentinel', sent(img[16 * M:])),
                ('rows of Ybar2, Ybar1 past the count keep their sentinel', sent(S[1:, 4 * M:]))]
    elif run.form == 'full':
        out.append(('rows of Ybar3, Ybar2, Ybar1 past the count keep their sentinel', sent(S[:, 4 * M:])))
    else:
        out.append(('rows of slots 0 and 1 of scratch past the count keep their sentinel', sent(S[:2, 4 * M:])))
    return out


def x0_tangent_rows(run):
    """(stored tangent rows of X0, gate0 W0[:, i] as float32) [M, 3, 128] of a full image: equal bit for bit where the promise holds."""
    M = run.M
    want = warp_x0(run.pts[:M], run.P['W0'], run.P['b0'], run.X[0][:4 * M])[1].view(M, 4, 128)[:, 1:]
    return run.X[0][:4 * M].view(M, 4, 128)[:, 1:], want


def rgb_exact_promises(run):
    M = run.M
    sent = lambda t: bool((bits(t) == SENT).all())
    out = [('rows of acts past the count keep their sentinel', sent(run.H[:, M:])),
           ('rows of rgb past the count keep their sentinel', sent(run.rgb[M:])),
           ('rows of feat_grad past the count keep their sentinel', sent(run.feat_grad[M:])),
           ('feat_grad columns 57 .. 63 are zero (the products with the zero padding of W0)', bool((run.feat_grad[:M, RGB_IN:] == 0).all())),
           ('the gradient of the padding columns of W0 is zero', bool((run.G['W0'][:, RGB_IN:] == 0).all()))]
    n = 3 if run.form == 'full' else 2
    out.append(('rows of scratch past the count keep their sentinel', sent(run.S[:n, M:])))
    return out


# -------------------------------------------------------------------------------------- float32 in a third association (CPU)
def _mm3(a, b):
    """a [m, k] @ b [k, n] in float32 numpy, K in four interleaved quarters whose sums are added in pairs."""
    p = [a[:, c::4] @ b[c::4] for c in range(4)]
    return (p[0] + p[1]) + (p[2] + p[3])


def _tn3(y, x):
    """y^T x in float32 numpy: 64-row blocks added in order."""
    acc = np.zeros((y.shape[1], x.shape[1]), np.float32)
    for m0 in range(0, y.shape[0], 64):
        acc += y[m0:m0 + 64].T @ x[m0:m0 + 64]
    return acc


def _sum3(y):
    acc = np.zeros(y.shape[1:], np.float32)
    for m0 in range(0, y.shape[0], 64):
        acc += y[m0:m0 + 64].sum(0, dtype=np.float32)
    return acc


def _sentinel(n):
    return torch.full((n,), SENT, dtype=torch.int32).view(F32)


def emulate32_warp(case, form='full'):
    """A whole forward + backward pass of the warp net in float32 numpy, every stage on its own stored inputs, products by _mm3 /
    _tn3 - neither the kernels' association nor torch's.  -> a run (make_warp_run) laid out as the kernels lay it out."""
    f = np.float32
    M, cap = min(int(case['count']), int(case['cap'])), int(case['cap'])
    flat = torch.tensor(case['flat'])
    P = {k: v.numpy() for k, v in warp_param_views(flat).items()}
    na, ns = workspace_floats(cap)['warp']
    acts, scr, grad = _sentinel(na), _sentinel(ns), torch.zeros_like(flat)
    X, S, G = warp_acts_view(acts, cap).numpy(), warp_scratch_view(scr, cap).numpy(), {k: v.numpy() for k, v in warp_param_views(grad).items()}
    pts, og, rng = np.asarray(case['pts'], f), np.asarray(case['out_grad'], f), f(case['out_range'])
    out, prefill = _sentinel(cap * 16).view(cap, 16), torch.tensor(np.asarray(case['prefill'], f))
    pg = prefill.clone()
    prim = (np.arange(4 * M) % 4 == 0)[:, None]
    y0 = _mm3(np.concatenate([pts[:M], np.ones((M, 1), f)], 1), np.concatenate([P['W0'], P['b0'][:, None]], 1).T.copy())
    g0 = y0 > 0
    x0 = np.concatenate([np.maximum(y0, f(0))[:, None], np.where(g0[:, None, :], P['W0'].T[None], f(0))], 1).reshape(4 * M, 128).astype(f)
    if form == 'lean':
        X[0][:4 * M:4] = x0[::4]
    else:
        X[0][:4 * M] = x0
    xs = [x0]
    for l in (1, 2, 3):
        y = _mm3(xs[-1], P[f'W{l}'].T.copy()) + P[f'b{l}'] * prim
        xs.append(np.where(np.repeat(y[::4] > 0, 4, 0), y, f(0)).astype(f))
        X[l][:4 * M] = xs[-1]
    out.numpy()[:M] = ((_mm3(xs[3], P['W4'].T.copy()) + P['b4'] * prim) * rng).reshape(M, 16)
    gate = lambda x: np.repeat(x[::4] > 0, 4, 0)
    g = (og[:M] * rng).reshape(4 * M, 4).astype(f)
    y3 = ((g[:, :2] @ P['W4'][:2] + g[:, 2:] @ P['W4'][2:]) * gate(xs[3])).astype(f)
    y2 = (_mm3(y3, P['W3']) * gate(xs[2])).astype(f)
    y1 = (_mm3(y2, P['W2']) * gate(xs[1])).astype(f)
    y0b = (_mm3(y1, P['W1']) * gate(xs[0])).astype(f)
    if form == 'lean':
        S[0].reshape(-1)[:16 * M] = g.reshape(-1)
    elif form == 'full':
        S[0][:4 * M] = y3
    if form == 'layered':
        S[0][:4 * M], S[1][:4 * M] = y1, y0b
    else:
        S[1][:4 * M], S[2][:4 * M] = y2, y1
    pg.numpy()[:M] += _mm3(y0b[::4], P['W0'])
    G['W4'][:], G['b4'][:] = _tn3(g, xs[3]), _sum3(g[::4])
    for l, y in ((3, y3), (2, y2), (1, y1)):
        G[f'W{l}'][:], G[f'b{l}'][:] = _tn3(y, xs[l - 1]), _sum3(y[::4])
    G['W0'][:] = _tn3(y0b[::4], pts[:M]) + _sum3(y0b.reshape(M, 4, 128)[:, 1:]).T
    G['b0'][:] = _sum3(y0b[::4])
    return make_warp_run(form, flat, grad, acts, scr, out, torch.tensor(pts), torch.tensor(og), pg, prefill, M, cap, rng)


def emulate32_rgb(case, form='full'):
    f = np.float32
    M, cap = min(int(case['count']), int(case['cap'])), int(case['cap'])
    flat = torch.tensor(case['flat'])
    P = {k: v.numpy() for k, v in rgb_param_views(flat).items()}
    na, ns = workspace_floats(cap)['rgbnet']
    acts, scr, grad = _sentinel(na), _sentinel(ns), torch.zeros_like(flat)
    H, S, G = rgb_acts_view(acts, cap).numpy(), rgb_scratch_view(scr, cap).numpy(), {k: v.numpy() for k, v in rgb_param_views(grad).items()}
    feat, gr = np.asarray(case['feat'], f), np.asarray(case['rgb_grad'], f)
    rgb, fg = _sentinel(cap * 3).view(cap, 3), _sentinel(cap * 64).view(cap, 64)
    x = feat[:M]
    for l in range(3):
        H[l][:M] = np.maximum(_mm3(x, P[f'W{l}'].T.copy()) + P[f'b{l}'], f(0))
        x = H[l][:M]
    s = _mm3(x, P['W3'].T.copy()) + P['b3']
    with np.errstate(over='ignore'):                         # exp(-s) = inf: the colour is 0
        c = (f(1) / (f(1) + np.exp(-s, dtype=f))).astype(f)
    rgb.numpy()[:M] = c
    gl = ((gr[:M] * (f(1) - c)) * c).astype(f)
    y2 = ((gl[:, :1] * P['W3'][:1] + gl[:, 1:] @ P['W3'][1:]) * (H[2][:M] > 0)).astype(f)
    y1 = (_mm3(y2, P['W2']) * (H[1][:M] > 0)).astype(f)
    y0 = (_mm3(y1, P['W1']) * (H[0][:M] > 0)).astype(f)
    if form == 'full':
        S[0][:M], S[1][:M], S[2][:M] = y2, y1, y0
    else:
        S[0][:M], S[1][:M] = y0, y1
    fg.numpy()[:M] = _mm3(y0, P['W0'])
    G['W3'][:], G['b3'][:] = _tn3(gl, H[2][:M]), _sum3(gl)
    for l, y in ((2, y2), (1, y1), (0, y0)):
        G[f'W{l}'][:], G[f'b{l}'][:] = _tn3(y, feat[:M] if l == 0 else H[l - 1][:M]), _sum3(y)
    return make_rgb_run(form, flat, grad, acts, scr, rgb, torch.tensor(feat), torch.tensor(gr), fg, M, cap)
