"""The scene branch's MLP chain (csrc/pp_nerf.hip: pp_nerf_fwd / pp_nerf_bwd) stage by stage: views of the two blocks the kernels
leave behind, the two ReLU mask-plane layouts, and one float64 / float32 reference per stage (TEST INFRASTRUCTURE ONLY).

A pass keeps every intermediate: `acts` holds enc, a[0 .. 7], h, raw and the mask planes, `scratch` holds d7, dH, dEnc0, dEncS, dHsum,
dView and DY[0 .. 6].  Each stage is therefore compared with an evaluation of THAT STAGE ALONE on the kernel's own stored inputs, and
every ReLU gate of a reference is (stored activation > 0): no state can differ between kernel and reference, no row needs excusing,
and helpers.check applies to every entry.

Every stage function returns (ref64, ref32, scale): the expression in float64, the same expression in torch float32 (a blocked
library product: another association than the kernels'), and the summed magnitudes of the terms behind an entry - for a product
sum_k |a_k| |b_k| (+ |bias|), for a weight gradient sum_m |dY| |x|, for an elementwise stage |value|.  Two stages carry a reasoned
scale of their own:
  rgb = sigmoid(s), s = R1 h + br1: |value| + sigmoid'(s) (sum |h| |R1| + |br1|) - the rounding of s, carried through the slope;
  g_center / g_ray: the sum over a ray's samples of |g_j| |d enc_j / d x_c| (times |depth| for the ray), plus the absolute terms
  of the view path through the normalisation.
tests/test_scene_mlp_reference.py ties the chained float64 stages to oracle.scene_nerf.mlp and its autograd gradients (1e-12) and
measures what a float32 evaluation in a third association (`emulate32`) needs under the rule.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import scene_nerf as SN
from tests.scene_ray_reference import ulps_needed  # noqa: F401  (re-exported: the tests print what each stage needs)

F64, F32 = torch.float64, torch.float32
IN_LD = (64, 256, 256, 256, 320, 256, 256, 256)             # row strides of the weights = input widths read (nerf_layout)
OUT_LD = (256, 256, 256, 320, 256, 256, 256, 288)           # row strides of the stored activations (nerf_acts)
MX_SLOTS, PART_FLOATS = 64, 512 * 392
PADDING = {'W0': (63,), 'W4': (319,), 'R0': (283, 284, 285, 286, 287)}       # columns of the parameter block no input reaches
PARAM_NAMES = tuple(n for l in range(8) for n in (f'W{l}', f'b{l}')) + ('wd', 'bd', 'R0', 'br0', 'R1', 'br1')


# ------------------------------------------------------------------------------------------------------------------- layouts
def param_offsets():
    """nerf_layout restated: [W0, b0, ..., W7, b7, wd, bd, R0, br0, R1, br1, total] in floats, the order of ops.nerf_layout()."""
    o, w, b = 0, [], []
    for l in range(7):
        w.append(o)
        o += 256 * IN_LD[l]
        b.append(o)
        o += 256
    wd, o = o, o + 256                                       # the density row sits in front of W7's rows, bd in front of b7
    w.append(o)
    o += 256 * 256
    bd, o = o, o + 1
    b.append(o)
    o += 256 + 63
    r0, o = o, o + 128 * 288
    br0, o = o, o + 128
    r1, o = o, o + 3 * 128
    br1, o = o, o + 64
    return [x for pair in zip(w, b) for x in pair] + [wd, bd, r0, br0, r1, br1, o]


def param_views(flat):
    """{name: view} of a packed parameter (or gradient) block, padding columns included: W_l [256, IN_LD[l]], b_l [256], wd [256],
    bd [1], R0 [128, 288], br0 [128], R1 [3, 128], br1 [3]."""
    off = param_offsets()
    P = {}
    for l in range(8):
        P[f'W{l}'] = flat[off[2 * l]:off[2 * l] + 256 * IN_LD[l]].view(256, IN_LD[l])
        P[f'b{l}'] = flat[off[2 * l + 1]:off[2 * l + 1] + 256]
    P['wd'], P['bd'] = flat[off[16]:off[16] + 256], flat[off[17]:off[17] + 1]
    P['R0'], P['br0'] = flat[off[18]:off[18] + 128 * 288].view(128, 288), flat[off[19]:off[19] + 128]
    P['R1'], P['br1'] = flat[off[20]:off[20] + 384].view(3, 128), flat[off[21]:off[21] + 3]
    return P


class _Walk:
    def __init__(self, base):
        self.base, self.o = base, 0

    def take(self, n, *shape):
        v = None if self.base is None else self.base[self.o:self.o + n]
        self.o += n
        return v if v is None or not shape else v[:math.prod(shape)].view(*shape)


def acts_views(acts, M):
    """nerf_acts restated.  acts = None: only ['end'], the size of the block, means anything."""
    w, V = _Walk(acts), {}
    V['enc'] = w.take(M * 64, M, 64)
    for l in range(8):
        V[f'a{l}'] = w.take(M * OUT_LD[l], M, OUT_LD[l])
    V['h'] = w.take(M * 128, M, 128)
    V['raw'] = w.take(M)
    V['mx'] = w.take(MX_SLOTS)
    Mp = (M + 127) // 128 * 128
    for l in range(8):
        V[f'bits{l}'] = w.take(Mp * 8)                      # one bit per activation: 32 bytes per (padded) row
    for l in range(8):
        V[f'wimg{l}'] = w.take(256 * IN_LD[l])              # fp16 hi + lo = 4 bytes per weight
    V['whead'] = w.take(10 * 8192)                          # the fused chain's ninth stage in its weight stream
    V['end'] = w.o
    return V


def scratch_views(scratch, M, R):
    """nerf_scratch restated.  d7 is [M, 288] and dH [M, 128], each at the head of an [M, 320] block."""
    w, V = _Walk(scratch), {}
    V['d7'] = w.take(M * 320, M, 288)
    V['dH'] = w.take(M * 320, M, 128)
    V['dEnc0'] = w.take(M * 64, M, 64)
    V['dEncS'] = w.take(M * 64, M, 64)
    V['dHsum'] = w.take(R * 128, R, 128)
    V['dView'] = w.take(R * 32, R, 32)
    for l in range(8):
        V[f'WT{l}'] = w.take(256 * (288 if l == 7 else IN_LD[l]))
    V['R0T'] = w.take(288 * 128)
    V['r0t_img'], V['wt7_img'] = w.take(256 * 128), w.take(256 * 288)
    for l in range(1, 7):
        V[f'wt_img{l}'] = w.take(256 * 256)
    V['part'] = w.take(PART_FLOATS)
    for l in range(7):
        V[f'DY{l}'] = w.take(M * 256, M, 256)
    V['end'] = w.o
    return V


def workspace_floats(M, R):
    return acts_views(None, M)['end'], scratch_views(None, M, R)['end']


# ------------------------------------------------------------------------------------------------------------ mask planes
_J = torch.arange(16)


def _plane_rows(dev):
    j = _J.to(dev)
    return ((j & 3) + 8 * (j >> 2))[None, :] + 4 * torch.arange(2, device=dev)[:, None]          # [half, j]


def mask_states_rows(b, M):
    """One mask plane of the fused chains' layout (int32 view: [row][column block][lane half] 16-bit words, bit j <-> column
    32 block + 4 half + (j & 3) + 8 (j >> 2)) -> [M, 256] bool."""
    Mp, dev = (M + 127) // 128 * 128, b.device
    wds = torch.stack([b & 0xFFFF, (b >> 16) & 0xFFFF], -1).view(Mp, 8, 2)                   # [row][w][half]
    j = torch.arange(16, device=dev)
    bits = ((wds[..., None] >> j) & 1).bool()                                                  # [row, w, half, j]
    col = (32 * torch.arange(8, device=dev)[:, None, None] + 4 * torch.arange(2, device=dev)[None, :, None]
           + ((j & 3) + 8 * (j >> 2))[None, None, :]).reshape(-1)
    out = torch.zeros(Mp, 256, dtype=torch.bool, device=dev)
    out[:, col] = bits.reshape(Mp, 256)
    return out[:M]


def mask_states_cols(b, M):
    """One mask plane of the layer-by-layer layout (int32 view: word [row group of 32][column][half] (16 bits), bit j <-> row
    32 g + (j & 3) + 8 (j >> 2) + 4 half) -> [M, 256] bool."""
    Mp, dev = (M + 127) // 128 * 128, b.device
    wds = torch.stack([b & 0xFFFF, (b >> 16) & 0xFFFF], -1).view(Mp // 32, 256, 2)
    j = torch.arange(16, device=dev)
    bits = ((wds[..., None] >> j) & 1).bool()                 # [g, col, half, j]
    out = torch.zeros(Mp // 32, 32, 256, dtype=torch.bool, device=dev)
    out[:, _plane_rows(dev).reshape(-1), :] = bits.permute(0, 2, 3, 1).reshape(Mp // 32, 32, 256)
    return out.view(Mp, 256)[:M]


def mask_pack_cols(st):
    """[M, 256] bool -> one mask plane of the layer-by-layer layout, as int64 values of its 32-bit words [row group of 32][column]."""
    M, dev = st.shape[0], st.device
    Mp = (M + 127) // 128 * 128
    full = torch.zeros(Mp, 256, dtype=torch.bool, device=dev)
    full[:M] = st
    j = torch.arange(16, device=dev)
    x = full.view(Mp // 32, 32, 256)[:, _plane_rows(dev).reshape(-1), :].view(Mp // 32, 2, 16, 256)   # [g, half, j, col]
    wds = (x.to(torch.int64) << j[None, None, :, None]).sum(2)                                    # [g, half, col]
    return (wds[:, 0] | (wds[:, 1] << 16)).to(torch.int64).view(-1)                              # [g * 256 + col]


# ---------------------------------------------------------------------------------------------------------- stage references
def _t(x, dt):
    return torch.as_tensor(x).to(dt)


def _three(expr, *xs, gate=None, post=None):
    """(expr in float64, expr in float32, expr on the magnitudes): for a sum of products the third is sum |a| |b|."""
    x64 = [_t(x, F64) for x in xs]
    r64, r32, sc = expr(*x64), expr(*[_t(x, F32) for x in xs]), expr(*[x.abs() for x in x64])
    if post is not None:
        r64, r32 = post(r64), post(r32)
    if gate is not None:
        r64, r32 = r64 * gate.to(F64), r32 * gate.to(F32)
    return r64, r32, sc


def layer(x, W, b):
    """relu(W x + b): x [M, K], W [256 | 128, K], K the true input width (64, 256, 320 or 288) with its padding columns."""
    return _three(lambda x, W, b: x @ W.T + b, x, W, b, post=torch.relu)


def raw_density(a6, wd, bd):
    return _three(lambda a, w, b: a @ w + b, a6[:, :256], wd, bd)


def _softplus(x):
    return torch.where(x > 20, x, torch.log1p(torch.exp(torch.clamp(x, max=20.0))))


def density(raw):
    """softplus(raw) with its > 20 branch, on the stored raw."""
    r64, r32 = _softplus(_t(raw, F64)), _softplus(_t(raw, F32))
    return r64, r32, r64.abs()


def rgb(h, R1, br1):
    s64, s32, ssc = _three(lambda h, W, b: h @ W.T + b, h, R1, br1)
    r64, r32 = torch.sigmoid(s64), torch.sigmoid(s32)
    return r64, r32, r64 + r64 * (1 - r64) * ssc


def _gl(g, c):
    return g * c * (1 - c)                                   # d loss / d (pre-sigmoid), on the stored colours c in [0, 1]


def d_hidden(g_rgb, rgb_s, R1, h):
    """dH = [h > 0] (gl R1), gl = g_rgb rgb (1 - rgb)."""
    return _three(lambda g, c, W: _gl(g, c) @ W, g_rgb, rgb_s, R1, gate=torch.as_tensor(h) > 0)


def grad_R1(g_rgb, rgb_s, h):
    return _three(lambda g, c, h: _gl(g, c).T @ h, g_rgb, rgb_s, h)


def grad_br1(g_rgb, rgb_s):
    return _three(lambda g, c: _gl(g, c).sum(0), g_rgb, rgb_s)


def grad_w(Y, X):
    """Y^T X: the gradient of the weights between X [M, K] and the output gradient Y [M, N]."""
    return _three(lambda Y, X: Y.T @ X, Y, X)


def grad_b(Y):
    return _three(lambda Y: Y.sum(0), Y)


def ray_sum(dH, R, S):
    return _three(lambda d: d.view(R, S, -1).sum(1), dH)


def d_view(dHsum, R0):
    return _three(lambda d, W: d @ W[:, 256:288], dHsum, R0)


def _dsoftplus(g, x):
    return g * torch.where(x > 20, torch.ones_like(x), torch.sigmoid(x))


def d_raw(g_density, raw):
    """Column 256 of d7: g_density softplus'(raw), with the > 20 branch."""
    r64, r32 = _dsoftplus(_t(g_density, F64), _t(raw, F64)), _dsoftplus(_t(g_density, F32), _t(raw, F32))
    return r64, r32, r64.abs()


def grad_wd(draw, a6):
    return _three(lambda g, a: g @ a, draw, a6[:, :256])


def grad_bd(draw):
    return _three(lambda g: g.sum(0, keepdim=True), draw)


def data_grad(Y, W, act):
    """[act > 0] (Y W): Y [M, N], W [N, K] (the columns of the weights that reach the activation `act` [M, K])."""
    return _three(lambda Y, W: Y @ W, Y, W, gate=torch.as_tensor(act) > 0)


def d_enc(Y, W):
    return _three(lambda Y, W: Y @ W, Y, W)


def _enc_jacobian_abs(x, L, w):
    """|d enc_j / d x_c| summed per coordinate needs the entries: [..., 3, 2 L + 1] magnitudes (raw, sines, cosines) of coordinate c."""
    f = (2.0 ** torch.arange(L, dtype=F64, device=x.device)) * math.pi
    ph = x[..., None] * f
    return torch.cat([torch.ones_like(x[..., None]), (f * w * ph.cos()).abs(), (f * w * ph.sin()).abs()], -1)


def ray_grads(center, ray, depth, bands, dEnc0, dEncS, dView):
    """g_center, g_ray [R, 3] as autograd of oracle.scene_nerf.encode (points) and of the normalised view direction, contracted with
    the stored dEnc0 + dEncS [M, 64] and dView [R, 32].  -> (g_center triple, g_ray triple)."""
    R, S = depth.shape
    res = []
    for dt in (F64, F32):
        c, r = _t(center, dt).clone().requires_grad_(True), _t(ray, dt).clone().requires_grad_(True)
        t, w = _t(depth, dt), _t(bands, dt)
        g = (_t(dEnc0, dt) + _t(dEncS, dt)).view(R, S, 64)
        pts = c[:, None] + r[:, None] * t[..., None]
        e = SN.encode(pts, SN.L_3D, w[:SN.L_3D])
        unit = r / r.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        ve = SN.encode(unit, SN.L_VIEW, w[SN.L_3D:])
        ((e * g[..., :63]).sum() + (ve * _t(dView, dt)[:, :27]).sum()).backward()
        res.append((c.grad, r.grad))
    # scales
    c, r, t, w = (_t(a, F64) for a in (center, ray, depth, bands))
    g = (_t(dEnc0, F64).abs() + _t(dEncS, F64).abs()).view(R, S, 64)
    gv = _t(dView, F64).abs()
    pts = c[:, None] + r[:, None] * t[..., None]
    L = SN.L_3D
    J = _enc_jacobian_abs(pts, L, w[:L])                                              # [R, S, 3, 1 + 2 L]: raw, d sin, d cos
    gq = torch.cat([g[..., :3, None], g[..., 3:63].reshape(R, S, 3, 2 * L)], -1)
    A = (gq * J).sum(-1)                                                              # [R, S, 3]
    n = r.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = r / n
    Lv = SN.L_VIEW
    Jv = _enc_jacobian_abs(u, Lv, w[L:])
    gu = (torch.cat([gv[:, :3, None], gv[:, 3:27].reshape(R, 3, 2 * Lv)], -1) * Jv).sum(-1)      # [R, 3]
    view = (gu + u.abs() * (u.abs() * gu).sum(-1, keepdim=True)) / n
    s_c, s_r = A.sum(1), (A * t[..., None].abs()).sum(1) + view
    return (res[0][0], res[1][0], s_c), (res[0][1], res[1][1], s_r)


# -------------------------------------------------------------------------------------------------------------- a finished pass
def make_run(flat, grad, acts, scratch, rgb_s, dens, g_rgb, g_den, g_center, g_ray, center, ray, depth, bands):
    """Everything a forward + backward pass read and left behind, as views (torch tensors of one device)."""
    R, S = depth.shape
    M = R * S
    return SimpleNamespace(R=R, S=S, M=M, P=param_views(flat), G=param_views(grad), A=acts_views(acts, M), X=scratch_views(scratch, M, R),
                           rgb=rgb_s.view(M, 3), density=dens.view(M), g_rgb=g_rgb.view(M, 3), g_den=g_den.view(M), g_center=g_center,
                           g_ray=g_ray, center=center, ray=ray, depth=depth, bands=bands)


def forward_stages(run, rows=None):
    """-> (name, the pass's value, (ref64, ref32, scale)) per forward stage; rows: a row subset (the stages are row-independent)."""
    P, A = run.P, run.A
    sl = (lambda x: x) if rows is None else (lambda x: x[rows])
    x = sl(A['enc'])
    for l in range(8):
        yield f'a{l}', sl(A[f'a{l}'])[:, :256], layer(x[:, :IN_LD[l]], P[f'W{l}'], P[f'b{l}'])
        x = sl(A[f'a{l}'])
    yield 'raw', sl(A['raw']), raw_density(sl(A['a6']), P['wd'], P['bd'])
    yield 'density', sl(run.density), density(sl(A['raw']))
    yield 'h', sl(A['h']), layer(sl(A['a7']), P['R0'], P['br0'])
    yield 'rgb', sl(run.rgb), rgb(sl(A['h']), P['R1'], P['br1'])


def data_gradient_stages(run, rows=None, names=None):
    """The row-independent backward stages: dH, d7 (its density column included), DY[6 .. 0], dEncS, dEnc0; names: only those."""
    P, A, X = run.P, run.A, run.X
    sl = (lambda x: x) if rows is None else (lambda x: x[rows])
    want = lambda n: names is None or n in names
    if want('dH'):
        yield 'dH', sl(X['dH']), d_hidden(sl(run.g_rgb), sl(run.rgb), P['R1'], sl(A['h']))
    if want('d7[:,256]'):
        yield 'd7[:,256]', sl(X['d7'])[:, 256], d_raw(sl(run.g_den), sl(A['raw']))
    if want('d7[:,:256]'):
        yield 'd7[:,:256]', sl(X['d7'])[:, :256], data_grad(sl(X['dH']), P['R0'][:, :256], sl(A['a7'])[:, :256])
    W7d = torch.cat([P['W7'], P['wd'][None]], 0)                                      # [257, 256]: the density row behind W7's
    if want('DY6'):
        yield 'DY6', sl(X['DY6']), data_grad(sl(X['d7'])[:, :257], W7d, sl(A['a6']))
    for l in range(6, 0, -1):
        if want(f'DY{l - 1}'):
            yield f'DY{l - 1}', sl(X[f'DY{l - 1}']), data_grad(sl(X[f'DY{l}']), P[f'W{l}'][:, :256], sl(A[f'a{l - 1}'])[:, :256])
    if want('dEncS'):
        yield 'dEncS', sl(X['dEncS']), d_enc(sl(X['DY4']), P['W4'][:, 256:320])
    if want('dEnc0'):
        yield 'dEnc0', sl(X['dEnc0']), d_enc(sl(X['DY0']), P['W0'])


def head_sum_stages(run):
    """The heads' parameter gradients, dHsum and dView: sums over all rows."""
    P, A, X, G = run.P, run.A, run.X, run.G
    yield 'g.R1', G['R1'], grad_R1(run.g_rgb, run.rgb, A['h'])
    yield 'g.br1', G['br1'], grad_br1(run.g_rgb, run.rgb)
    yield 'g.wd', G['wd'], grad_wd(X['d7'][:, 256], A['a6'])
    yield 'g.bd', G['bd'], grad_bd(X['d7'][:, 256])
    yield 'dHsum', X['dHsum'], ray_sum(X['dH'], run.R, run.S)
    yield 'dView', X['dView'], d_view(X['dHsum'], P['R0'])


def weight_gradient_stages(run):
    """The nine weight-gradient products with their bias sums: R0, W7 .. W0."""
    A, X, G = run.A, run.X, run.G
    yield 'g.R0', G['R0'], grad_w(X['dH'], A['a7'])
    yield 'g.br0', G['br0'], grad_b(X['dH'])
    yield 'g.W7', G['W7'], grad_w(X['d7'][:, :256], A['a6'])
    yield 'g.b7', G['b7'], grad_b(X['d7'][:, :256])
    for l in range(6, -1, -1):
        xin = A['enc'] if l == 0 else A[f'a{l - 1}'][:, :IN_LD[l]]
        yield f'g.W{l}', G[f'W{l}'], grad_w(X[f'DY{l}'], xin)
        yield f'g.b{l}', G[f'b{l}'], grad_b(X[f'DY{l}'])


def ray_gradient_stages(run, rays=None):
    X = run.X
    R, S = run.R, run.S
    if rays is None:
        rays = torch.arange(R, device=run.depth.device)
    m = (rays[:, None] * S + torch.arange(S, device=rays.device)[None]).reshape(-1)
    cpu = lambda t: t.detach().cpu()                          # (oracle.scene_nerf.encode builds its frequencies on the CPU)
    gc, gr = ray_grads(cpu(run.center[rays]), cpu(run.ray[rays]), cpu(run.depth[rays]), cpu(run.bands), cpu(X['dEnc0'][m]),
                       cpu(X['dEncS'][m]), cpu(X['dView'][rays]))
    yield 'g_center', run.g_center[rays], gc
    yield 'g_ray', run.g_ray[rays], gr


def all_stages(run):
    for gen in (forward_stages, data_gradient_stages, head_sum_stages, weight_gradient_stages, ray_gradient_stages):
        yield from gen(run)


def exact_promises(run):
    """What holds bit for bit whatever the route: -> list of (what, bool)."""
    A, X, G = run.A, run.X, run.G
    out = [('skip copy a3[:,256:320] == enc', torch.equal(A['a3'][:, 256:], A['enc'])),
           ('enc column 63 == 0', bool((A['enc'][:, 63] == 0).all())),
           ('view columns 283 .. 287 of a7 == 0', bool((A['a7'][:, 283:] == 0).all())),
           ('d7 columns 257 .. 287 == 0', bool((X['d7'][:, 257:] == 0).all()))]
    for name, cols in PADDING.items():
        out.append((f'gradient of the padding columns of {name} == 0', bool((G[name][:, list(cols)] == 0).all())))
    return out


def mask_planes(run, rows_layout):
    """-> the eight [M, 256] bool planes of the pass, unpacked from the layout its route writes."""
    unpack = mask_states_rows if rows_layout else mask_states_cols
    return [unpack(run.A[f'bits{l}'].view(torch.int32), run.M) for l in range(8)]


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


def emulate32(case, forward_only=False):
    """A whole forward + backward pass in float32 numpy, every stage on its own stored inputs, products by _mm3 / _tn3 - neither the
    kernels' association nor torch's.  -> a run (make_run) whose blocks are laid out as the kernels lay them out."""
    f = np.float32
    R, S = case['depth'].shape
    M = R * S
    flat = torch.tensor(case['flat'])
    P = {k: v.numpy() for k, v in param_views(flat).items()}
    n_acts, n_scr = workspace_floats(M, R)
    acts, scr, grad = torch.zeros(n_acts), torch.zeros(n_scr), torch.zeros_like(flat)
    A = {k: (v.numpy() if v is not None else None) for k, v in acts_views(acts, M).items() if k != 'end'}
    X = {k: (v.numpy() if v is not None else None) for k, v in scratch_views(scr, M, R).items() if k != 'end'}
    G = {k: v.numpy() for k, v in param_views(grad).items()}
    center, ray, depth, bands = (torch.tensor(case[k]) for k in ('center', 'ray', 'depth', 'bands'))
    pts = center[:, None] + ray[:, None] * depth[..., None]
    unit = ray / ray.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    A['enc'][:, :63] = SN.encode(pts, SN.L_3D, bands[:SN.L_3D]).reshape(M, 63).numpy()
    A['a3'][:, 256:] = A['enc']
    A['a7'][:, 256:283] = np.repeat(SN.encode(unit, SN.L_VIEW, bands[SN.L_3D:]).numpy(), S, 0)
    x = A['enc']
    for l in range(8):
        A[f'a{l}'][:, :256] = np.maximum(_mm3(x[:, :IN_LD[l]], P[f'W{l}'].T.copy()) + P[f'b{l}'], f(0))
        x = A[f'a{l}']
    A['raw'][:] = _mm3(A['a6'], P['wd'][:, None].copy())[:, 0] + P['bd']
    raw = A['raw']
    dens = np.where(raw > 20, raw, np.log1p(np.exp(np.minimum(raw, f(20)), dtype=f), dtype=f)).astype(f)
    A['h'][:] = np.maximum(_mm3(A['a7'], P['R0'].T.copy()) + P['br0'], f(0))
    rgb_s = (f(1) / (f(1) + np.exp(-(_mm3(A['h'], P['R1'].T.copy()) + P['br1']), dtype=f))).astype(f)
    g_rgb, g_den = np.asarray(case['g_rgb'], f), np.asarray(case['g_den'], f)
    tt = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=f))
    if forward_only:
        return make_run(flat, grad, acts, scr, tt(rgb_s), tt(dens), tt(g_rgb), tt(g_den), torch.zeros(R, 3), torch.zeros(R, 3), center, ray,
                        depth, bands)
    gl = (g_rgb * (f(1) - rgb_s)) * rgb_s
    X['dH'][:] = _mm3(gl, P['R1']) * (A['h'] > 0)
    G['R1'][:], G['br1'][:] = _tn3(gl, A['h']), _sum3(gl)
    G['R0'][:], G['br0'][:] = _tn3(X['dH'], A['a7']), _sum3(X['dH'])
    X['dHsum'][:] = X['dH'].reshape(R, S, 128)[:, ::-1].sum(1, dtype=f)
    X['dView'][:] = _mm3(X['dHsum'], P['R0'][:, 256:288].copy())
    X['d7'][:, 256] = g_den * np.where(raw > 20, f(1), f(1) / (f(1) + np.exp(-raw, dtype=f))).astype(f)
    G['wd'][:], G['bd'][:] = _tn3(X['d7'][:, 256:257], A['a6'])[0], _sum3(X['d7'][:, 256:257])
    X['d7'][:, :256] = _mm3(X['dH'], P['R0'][:, :256].copy()) * (A['a7'][:, :256] > 0)
    X['DY6'][:] = (_mm3(X['d7'][:, :256], P['W7']) + X['d7'][:, 256:257] * P['wd'][None]) * (A['a6'] > 0)
    for l in range(6, 0, -1):
        X[f'DY{l - 1}'][:] = _mm3(X[f'DY{l}'], P[f'W{l}'][:, :256].copy()) * (A[f'a{l - 1}'][:, :256] > 0)
    G['W7'][:], G['b7'][:] = _tn3(X['d7'][:, :256], A['a6']), _sum3(X['d7'][:, :256])
    for l in range(6, -1, -1):
        xin = A['enc'] if l == 0 else A[f'a{l - 1}'][:, :IN_LD[l]]
        G[f'W{l}'][:], G[f'b{l}'][:] = _tn3(X[f'DY{l}'], xin), _sum3(X[f'DY{l}'])
    X['dEncS'][:] = _mm3(X['DY4'], P['W4'][:, 256:320].copy())
    X['dEnc0'][:] = _mm3(X['DY0'], P['W0'])
    # the rays: the derivative from the STORED encoding (d sin = f cos: the partner element), as the kernel forms it
    g = (X['dEnc0'] + X['dEncS']).reshape(R, S, 64)
    e = A['enc'].reshape(R, S, 64)
    L = SN.L_3D
    fr = (np.pi * 2.0 ** np.arange(L)).astype(f)
    gq, eq = g[..., 3:63].reshape(R, S, 3, 2, L), e[..., 3:63].reshape(R, S, 3, 2, L)
    dp = g[..., :3] + ((gq[..., 0, :] * eq[..., 1, :] - gq[..., 1, :] * eq[..., 0, :]) * fr).sum(-1, dtype=f)      # [R, S, 3]
    g_center = dp.sum(1, dtype=f)
    t = np.asarray(case['depth'], f)
    gv, ve = X['dView'], A['a7'].reshape(R, S, 288)[:, 0, 256:]
    Lv = SN.L_VIEW
    gvq, veq = gv[:, 3:27].reshape(R, 3, 2, Lv), ve[:, 3:27].reshape(R, 3, 2, Lv)
    gu = gv[:, :3] + ((gvq[:, :, 0] * veq[:, :, 1] - gvq[:, :, 1] * veq[:, :, 0]) * fr[:Lv]).sum(-1, dtype=f)
    d = np.asarray(case['ray'], f)
    n = np.maximum(np.sqrt((d * d).sum(1, dtype=f)), f(1e-12))[:, None]
    u = d / n
    g_ray = (dp * t[..., None]).sum(1, dtype=f) + (gu - u * (u * gu).sum(1, keepdims=True, dtype=f)) / n
    return make_run(flat, grad, acts, scr, tt(rgb_s), tt(dens), tt(g_rgb), tt(g_den), tt(g_center), tt(g_ray), center, ray, depth, bands)
