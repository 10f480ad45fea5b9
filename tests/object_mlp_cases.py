"""Seeded inputs of tests/test_hip_object_mlp_kernels.py and tests/test_object_mlp_reference.py (numpy float32, no GPU): a packed
parameter block, inputs, upstream gradients, count and capacity of one pass of the warp net or of rgbnet.

Parameters are _warp_params(3) / _rgb_params(5) of tests/test_hip_mlp.py, so the magnitudes are those of the existing tests, with the
two scale pairs in use there: (1, 1), and weights x 1e-3 with gradients x 1e-6 times a per-sample magnitude exp(2 randn).
Planted cases (`plant`):
  'some_upstream' / 'no_upstream'   out_grad / rgb_grad rows all zero for every third sample / for all samples;
  'dead_silent'   units DEAD of hidden layer 2 (warp) / 1 (rgbnet) have a bias of -8 times the layer's largest float64 pre-activation
                  over the case's samples: dead for every sample; units SILENT have zero incoming weights and zero bias: y = +0
                  exactly, with zero tangents.  (The bias is large against the ACTIVATIONS, not in absolute terms: the split-precision
                  kernels take a tile's operand scale from the bound max|x| sum|W| + max|b|, so a bias 2^33 above the values - -1e3
                  beside weights x 1e-3 - puts the next layer's operand at its absolute floor: X3 was then 1.4 % off)
  'zero_gate'     (warp net) sample ZERO_SAMPLE has p = (0, 0, 0) and b0[n] = 0 for n in ZERO_UNITS, whose W0[n] are not zero: a
                  primal pre-activation of exactly +0 with non-zero tangents behind it;
  'range'         sample RANGE_SAMPLE (inside the second 32-row half) has inputs and gradients 2^20 times the others'."""
import numpy as np

from tests.object_mlp_reference import RGB_IN, RGB_SHAPES, WARP_SHAPES
from tests.test_hip_mlp import OUT_RANGE, _rgb_params, _warp_params

F32 = np.float32
SCALES = ((1.0, 1.0), (1e-3, 1e-6))
WARP_SIZES = (1, 7, 8, 9, 15, 16, 17, 16 * 3 + 7, 567)      # samples: around a 32-row half (8) and a 64-row tile (16)
RGB_SIZES = (1, 31, 32, 33, 63, 64, 65, 64 * 3 + 5, 2245)    # rows
PLANTS = ('some_upstream', 'no_upstream', 'dead_silent', 'zero_gate', 'range')
DEAD, SILENT = (5, 77, 120), (9, 64, 127)
ZERO_SAMPLE, ZERO_UNITS = 21, (3, 40, 41, 100)
RANGE_SAMPLE = {'warp': 12, 'rgbnet': 45}                    # rows 48 .. 51 / row 45: in the second half of the first tile
RANGE_FACTOR = 2.0 ** 20


def setting(i):
    """(scale pair, capacity - count) of the i-th size: the pairs alternate, every third size has a capacity above its count."""
    return SCALES[i % 2], (3 if i % 3 == 1 else 0)


def second_tile_sizes(cus):
    """The smallest sizes that give every work-group of the default grid (one per compute unit) a second tile, the last one ragged."""
    return 16 * cus + 16 + 7, 64 * cus + 64 + 5


def _pack(layers, shapes):
    out = []
    for (W, b), (n, k) in zip(layers, shapes):
        Wp = np.zeros((n, k), F32)
        Wp[:, :W.shape[1]] = W
        out += [Wp.reshape(-1), np.asarray(b, F32)]
    return np.concatenate(out)


def _largest_pre_activation(net, L, hid, x):
    """max |pre-activation| of hidden layer `hid` in float64 (primal rows), x: the case's inputs."""
    h = np.asarray(x, np.float64)
    for l in range(hid + 1):
        W = np.asarray(L[l][0], np.float64)
        y = h[:, :W.shape[1]] @ W.T + np.asarray(L[l][1], np.float64)
        h = np.maximum(y, 0.0)
    return float(np.abs(y).max())


def _layers(net, wscale, plant, x=None):
    if net == 'warp':
        L = [[(W * (wscale if 0 < i < 4 else 1.0)).numpy().copy(), (b * wscale).numpy().copy()] for i, (W, b) in enumerate(_warp_params(3))]
        hid = 2
    else:
        L = [[(W * (wscale if i < 3 else 1.0)).numpy().copy(), (b * wscale).numpy().copy()] for i, (W, b) in enumerate(_rgb_params(5))]
        hid = 1
    if plant == 'dead_silent':
        dead = -8.0 * _largest_pre_activation(net, L, hid, x)
        for n in DEAD:
            L[hid][1][n] = dead
        for n in SILENT:
            L[hid][0][n, :] = 0.0
            L[hid][1][n] = 0.0
    if plant == 'zero_gate':
        assert net == 'warp'
        for n in ZERO_UNITS:
            L[0][1][n] = 0.0
            assert (L[0][0][n] != 0).all()
    return L


def _upstream(rng, M, width, gscale, plant):
    g = rng.standard_normal((M, width)) * gscale
    if gscale != 1.0:
        g *= np.exp(2 * rng.standard_normal((M, 1)))
    if plant == 'some_upstream':
        g[::3] = 0.0
    if plant == 'no_upstream':
        g[:] = 0.0
    return g


def warp_case(M, cap=None, count=None, scales=SCALES[0], plant=None, seed=0):
    """-> dict: flat [WARP_PARAMS + 60], pts [cap, 3], out_grad [cap, 16], prefill [cap, 3] (pts_grad accumulates), count, cap,
    out_range.  M: the rows that carry data; cap >= M; count: what the kernels are told (default M; may exceed cap)."""
    cap = M if cap is None else cap
    rng = np.random.default_rng(7000 + 10 * M + seed)
    flat = np.zeros(sum(n * k + n for n, k in WARP_SHAPES) + 60, F32)
    pts = rng.standard_normal((cap, 3)) * 0.5
    P = _pack(_layers('warp', scales[0], plant, pts.astype(F32)), WARP_SHAPES)
    flat[:P.size] = P
    og = _upstream(rng, cap, 16, scales[1], plant)
    if plant == 'zero_gate':
        assert M > ZERO_SAMPLE
        pts[ZERO_SAMPLE] = 0.0
    if plant == 'range':
        assert M > RANGE_SAMPLE['warp']
        pts[RANGE_SAMPLE['warp']] *= RANGE_FACTOR
        og[RANGE_SAMPLE['warp']] *= RANGE_FACTOR
    out = dict(pts=pts, out_grad=og, prefill=rng.standard_normal((cap, 3)) * 0.25 * scales[1])
    out = {k: np.ascontiguousarray(v, dtype=F32) for k, v in out.items()}
    out.update(flat=flat, count=M if count is None else count, cap=cap, out_range=F32(OUT_RANGE))
    return out


def rgb_case(M, cap=None, count=None, scales=SCALES[0], plant=None, seed=0):
    """-> dict: flat [RGBNET_PARAMS + 60], feat [cap, 64] (columns 57 .. 63 zero), rgb_grad [cap, 3], count, cap."""
    cap = M if cap is None else cap
    rng = np.random.default_rng(9000 + 10 * M + seed)
    flat = np.zeros(sum(n * k + n for n, k in RGB_SHAPES) + 60, F32)
    feat = np.zeros((cap, 64))
    feat[:, :RGB_IN] = rng.standard_normal((cap, RGB_IN))
    P = _pack(_layers('rgbnet', scales[0], plant, feat.astype(F32)), RGB_SHAPES)
    flat[:P.size] = P
    gr = _upstream(rng, cap, 3, scales[1], plant)
    if plant == 'range':
        assert M > RANGE_SAMPLE['rgbnet']
        feat[RANGE_SAMPLE['rgbnet']] *= RANGE_FACTOR
        gr[RANGE_SAMPLE['rgbnet']] *= RANGE_FACTOR
    out = {k: np.ascontiguousarray(v, dtype=F32) for k, v in dict(feat=feat, rgb_grad=gr).items()}
    out.update(flat=flat, count=M if count is None else count, cap=cap)
    return out
