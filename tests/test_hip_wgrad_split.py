"""Split-precision weight-gradient chain (k_wgrad_chain_s, mlp_split bit 16) through both entry points, pp_warp_bwd_weights
(three 128 x 128 layers, bias sums over the primal rows of the 4-row form) and pp_rgbnet_bwd_weights (two 128 x 128 layers and
the 128 x 64 input layer, bias sums over every row), against float64 products of the same operands and against the fp32
chain kernel (bit 16 clear): ragged row counts, tile magnitudes that jump up and down, and a sentinel fence."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
WARP_BASE = 128 * 3 + 128                                       # W0, b0 in front of W1


def _layout(net, cap):
    """(rows of the chain, acts floats, scratch floats, params_grad floats, [(Wbar offset, KX, bias offset)] for the layers
    fed by Y[0], Y[1], Y[2], the Y/X tensors' acts / scratch slots)."""
    from poseprobe_amd import ops
    if net == 'warp':
        rc = cap * 4
        layers = [(WARP_BASE + l * (128 * 128 + 128), 128) for l in (2, 1, 0)]    # W3, W2, W1
        return rc, 4 * rc * 128, 3 * rc * 128 + 49152, ops.WARP_PARAMS + 60, layers
    rc = cap
    w1 = 128 * 64 + 128
    layers = [(w1 + 128 * 128 + 128, 128), (w1, 128), (0, 64)]                    # W2, W1, W0
    return rc, 3 * rc * 128, 3 * rc * 128 + 49152, ops.RGBNET_PARAMS + 60, layers


def _operands(net, M, cap, g, tile_exp=None):
    """Y[3] ([rows][128]) and X[3] ([rows][KX]) of the chain at M samples, and the flat buffers the entry points read."""
    rc, na, ns, _, layers = _layout(net, cap)
    rows = M * 4 if net == 'warp' else M
    Y = [torch.randn(rows, 128, generator=g) for _ in range(3)]
    X = [torch.relu(torch.randn(rows, kx, generator=g)) * torch.exp2(torch.randn(rows, 1, generator=g) * 2) for _, kx in layers]
    if net == 'rgbnet':
        X[2][:, 57:] = 0                                        # the padded input columns
    if tile_exp is not None:                                    # per 64-row tile magnitudes: Y x 2^e[0], X x 2^e[1]
        e = tile_exp.repeat_interleave(64, dim=0)[:rows]
        Y = [y * torch.exp2(e[:, :1]) for y in Y]
        X = [x * torch.exp2(e[:, 1:]) for x in X]
    acts = torch.zeros(na)
    scratch = torch.zeros(ns)
    feat = torch.zeros(cap, 64)
    for i in range(3):
        scratch[i * rc * 128:i * rc * 128 + rows * 128] = Y[i].reshape(-1)
    if net == 'warp':                                           # X of W3, W2, W1: acts[2], acts[1], acts[0]
        for i, slot in enumerate((2, 1, 0)):
            acts[slot * rc * 128:slot * rc * 128 + rows * 128] = X[i].reshape(-1)
    else:                                                       # X of W2, W1: acts[1], acts[0]; of W0: feat
        for i, slot in enumerate((1, 0)):
            acts[slot * rc * 128:slot * rc * 128 + rows * 128] = X[i].reshape(-1)
        feat[:rows] = X[2]
    return Y, X, acts.to(DEV), scratch.to(DEV), feat.to(DEV)


def _run(net, mode, acts, scratch, feat, count, cap, grad):
    from poseprobe_amd import ops
    cx = ops.Context(mlp_split=mode)
    if net == 'warp':
        ops.warp_bwd_weights(acts, scratch, count, cap, grad, 1, cx)
    else:
        ops.rgbnet_bwd_weights(feat, acts, scratch, count, cap, grad, 1, cx)
    torch.cuda.synchronize()


def _errors(net, M, cap, Y, X, acts, scratch, feat):
    """relative rms errors of the three Wbar against float64, fp32 chain and split chain; checks the bias sums of both."""
    from poseprobe_amd import _lib
    _, _, _, npg, layers = _layout(net, cap)
    count = torch.tensor([M], dtype=torch.int32, device=DEV)
    default = _lib.get_option('mlp_split')
    err = {}
    for mode in (default & ~16, default | 16):
        grad = torch.zeros(npg, device=DEV)
        _run(net, mode, acts, scratch, feat, count, cap, grad)
        e = []
        for i, (off, kx) in enumerate(layers):
            ref = Y[i].to(DEV).double().T @ X[i].to(DEV).double()
            got = grad[off:off + 128 * kx].view(128, kx).double()
            refb = Y[i][::4 if net == 'warp' else 1].to(DEV).double().sum(0)
            gb = grad[off + 128 * kx:off + 128 * kx + 128].double()
            assert float((gb - refb).abs().max()) <= 1e-5 * float(refb.abs().max()) + 1e-30, f'{net} bias {i}, mode {mode}'
            if net == 'rgbnet' and kx == 64:
                assert bool((got[:, 57:] == 0).all()), f'padded input columns, mode {mode}'
            den = float((ref ** 2).mean().sqrt())
            if den == 0.0:
                assert bool((got == 0).all()), f'{net} layer {i} at M = {M}, mode {mode}: nonzero gradient of no rows'
                e.append(0.0)
            else:
                e.append(float(((got - ref) ** 2).mean().sqrt()) / den)
        err[mode & 16] = e
    return err


def _assert_as_accurate(net, err, what, ratio=1.25):
    # the split products carry 22 significant bits: a sum of few rows, where fp32 rounds once, is allowed that floor
    for i, (a, b) in enumerate(zip(err[0], err[16])):
        assert b < 5e-6 and (b <= ratio * a + 1e-9 or b <= 4e-7), f'{net} layer {i} ({what}): fp32 chain {a:.3e}, split chain {b:.3e}'


@pytest.mark.parametrize('net', ['warp', 'rgbnet'])
@pytest.mark.parametrize('M,cap', [(0, 40), (1, 1), (63, 70), (65, 65), (16385, 16400), (54600, 54613)])
def test_split_weight_gradients_on_ragged_row_counts(net, M, cap):
    """R = 0 (every work-group empty), one row, less than a tile, a ragged second tile, 256 tiles + 1 (the last round's rows
    shared out in 16-row pieces) and the benchmark's sample count (warp: the whole grid at work, rgbnet: half of it).  At the benchmark's 218 k warp rows a work-group sums ~1300
    rows in fp32 and the split chain's error grows past the fp32 chain's: 1.34-1.37 x on these operands (the previous kernel,
    with half the work-groups: 1.76-1.82 x), so that size is held to 1.5 x."""
    g = torch.Generator().manual_seed(1000 + M)
    Y, X, acts, scratch, feat = _operands(net, M, cap, g)
    _assert_as_accurate(net, _errors(net, M, cap, Y, X, acts, scratch, feat), f'M = {M}', 1.5 if M * 4 > 100000 else 1.25)


def test_split_rgbnet_weight_gradients_with_every_work_group_at_work():
    """Below 8 tiles per work-group only the first half of the grid works; 100 k rgbnet rows are above it (the 128- and the
    64-wide layer with two work-groups per CU)."""
    M = 100000
    g = torch.Generator().manual_seed(99)
    Y, X, acts, scratch, feat = _operands('rgbnet', M, M, g)
    _assert_as_accurate('rgbnet', _errors('rgbnet', M, M, Y, X, acts, scratch, feat), f'M = {M}')


@pytest.mark.parametrize('net', ['warp', 'rgbnet'])
def test_split_weight_gradients_follow_tile_maxima_that_jump(net):
    """Every 64-row tile of Y is scaled by 2^-20, 2^0 or 2^20 and every tile of X by 2^-4 .. 2^4, in random order: the
    work-group's running exponents must be agreed on by all wavefronts and lowered - with a re-conversion of the tile - whenever
    a tile exceeds them, while tiles 2^40 smaller in between still count.  (One exponent per operand and work-group is the
    design's limit: where one operand sits 2^20 below its running maximum on exactly the rows where the other peaks, its
    products keep ~2^-17 of their value - 2e-5 relative, in this kernel as in its predecessor.)"""
    M = 6000
    rows = 4 * M if net == 'warp' else M
    g = torch.Generator().manual_seed(77)
    ntiles = (rows + 63) // 64
    tile_exp = torch.stack([(torch.randint(0, 3, (ntiles,), generator=g).float() - 1.0) * 20.0,
                            torch.randint(-4, 5, (ntiles,), generator=g).float()], 1)
    Y, X, acts, scratch, feat = _operands(net, M, M, g, tile_exp)
    _assert_as_accurate(net, _errors(net, M, M, Y, X, acts, scratch, feat), 'jumping tile maxima')


@pytest.mark.parametrize('net', ['warp', 'rgbnet'])
@pytest.mark.parametrize('M,cap', [(4099, 4099), (37, 50)])
def test_split_weight_gradients_stay_inside_their_buffers(net, M, cap):
    """The parameter-gradient block embedded in a sentinel arena: the sentinels around it survive, the entries that are not
    the three layers' Wbar / bbar stay zero, and the operands are not written."""
    from poseprobe_amd import _lib
    PAD = 16384
    SENT = 0x7FC0DEAD
    _, _, _, npg, layers = _layout(net, cap)
    g = torch.Generator().manual_seed(5)
    Y, X, acts, scratch, feat = _operands(net, M, cap, g)
    acts0, scratch0, feat0 = acts.clone(), scratch.clone(), feat.clone()
    arena = torch.empty(npg + 2 * PAD, dtype=torch.int32, device=DEV).fill_(SENT).view(torch.float32)
    grad = arena[PAD:PAD + npg]
    grad.zero_()
    count = torch.tensor([M], dtype=torch.int32, device=DEV)
    _run(net, _lib.get_option('mlp_split') | 16, acts, scratch, feat, count, cap, grad)
    a = arena.view(torch.int32)
    assert bool((a[:PAD] == SENT).all()), 'sentinels in front of the gradient block were overwritten'
    assert bool((a[PAD + npg:] == SENT).all()), 'sentinels behind the gradient block were overwritten'
    touched = torch.zeros(npg, dtype=torch.bool, device=DEV)
    for off, kx in layers:
        touched[off:off + 128 * kx + 128] = True
    assert bool((grad[~touched] == 0).all()), 'entries outside the three layers were written'
    assert torch.equal(acts, acts0) and torch.equal(scratch, scratch0) and torch.equal(feat, feat0), 'operands were written'
