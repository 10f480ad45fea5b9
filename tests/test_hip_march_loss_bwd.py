"""pp_march_loss_bwd: composite, ray losses and compositing backward of a ray by one wavefront in one launch, against
pp_march_fwd -> pp_loss_rays -> pp_march_bwd on the same inputs.  The fused kernel runs the same per-chunk and per-ray code on the
same values (kept in registers instead of read back): every per-sample and per-ray output has to be bit-identical.  Only the four
loss values are summed in another order (per work-group of four rays, then the rows in a fixed order by the last work-group to
arrive, instead of per 256 rays and float atomics); their tolerance is derived in LOSS_DISTANCE below.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CAP = 186                                       # samples of a ray in the benchmark scene and the most the test uses (three chunks)
W_MAIN, W_ENT, W_MASK, LS = 1.0, 0.01, 0.1, 0.1
SLOTS = (0, 1, 6, 7)                            # loss_out entries of the ray terms: mse, entropy, bce mask, weighted total
F32 = np.float32


def _ray(kind, n, g):
    """alpha of one ray of n samples.  'never': no early stop; 'first': stops inside the first chunk; 'boundary': the transmittance
    falls below 1e-3 exactly at sample 63, so i_end = 64, a chunk boundary; 'last': stops at the last sample but one, for more than
    130 samples in the last chunk; 'opaque': a sample with alpha = 1 (alphainv_last = 0, below its clamp range; when it is the first
    sample, cum_weights = 1, above its clamp range)."""
    a = torch.rand(n, generator=g) * 0.01
    if kind == 'first' and n > 0:
        a = torch.rand(n, generator=g) * 0.5 + 0.3
    elif kind == 'boundary' and n >= 64:
        a[:63] = 1e-4
        a[63] = 0.9995
    elif kind == 'last' and n > 1:
        a[n - 2] = 0.9995
    elif kind == 'opaque' and n > 0:
        a[int(torch.randint(0, min(n, 3), (1,), generator=g))] = 1.0
    return a


def make_case(name):
    g = torch.Generator().manual_seed({'seven': 11, 'many': 12}[name])
    if name == 'seven':
        lens = [0, 1, 63, 64, 65, 129, 186]
        kinds = ['never', 'opaque', 'first', 'never', 'boundary', 'never', 'last']
    else:
        lens = torch.randint(0, CAP + 1, (261,), generator=g).tolist()
        lens[:6] = [186, 64, 128, 0, 186, 70]
        pool = ['never', 'first', 'boundary', 'last', 'opaque']
        kinds = [pool[i % 5] for i in range(261)]
        kinds[0], kinds[1], kinds[2] = 'never', 'boundary', 'boundary'
    N = len(lens)
    rs = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    M = int(rs[-1])
    alpha = torch.cat([_ray(k, n, g) for k, n in zip(kinds, lens)])
    rgb = torch.rand(M, 3, generator=g)
    # a third of the rays composite a first channel below 0 and a second one above 1 (where their weights add up to enough): the
    # clamp mask zeroes those channels' gradients
    ray_of = torch.repeat_interleave(torch.arange(N), torch.tensor(lens))
    wild = (torch.arange(N) % 3 == 1)[ray_of]
    rgb[wild, 0] = -1.5 - rgb[wild, 0]
    rgb[wild, 1] = 2.0 + rgb[wild, 1]
    d = dict(N=N, M=M, rs=rs, alpha=alpha, rgb=rgb, step=torch.rand(M, generator=g) + 0.5, target=torch.rand(N, 3, generator=g),
             mask=(torch.arange(N) % 4 != 2).float(), lens=lens, kinds=kinds)
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


PER_SAMPLE = ('weights', 'T', 'g_alpha', 'g_rgb')
PER_RAY = ('alphainv_last', 'i_end', 'rgb_marched', 'rgb_pre', 'cum_weights', 'depth_acc', 'g_rgbm', 'g_last', 'g_cw', 'mask_sum')


def buffers(d):
    N, M = d['N'], d['M']
    f = lambda *s: torch.full(s, -77.0, device='cuda')
    return dict(weights=f(M + 64), T=f(M + 64), g_alpha=f(M + 64), g_rgb=f(M + 64, 3), alphainv_last=f(N), rgb_marched=f(N, 3),
                i_end=torch.full((N,), -7, dtype=torch.int32, device='cuda'), rgb_pre=f(N, 3), cum_weights=f(N), depth_acc=f(N),
                g_rgbm=f(N, 3), g_last=f(N), g_cw=f(N), mask_sum=f(1), loss=torch.zeros(8, device='cuda'))


def run_separate(d, bg):
    from poseprobe_amd import ops
    o = buffers(d)
    ops.march_fwd(d['alpha'], d['rgb'], d['step'], None, d['rs'], d['N'], bg, o['weights'], o['T'], o['alphainv_last'], o['i_end'],
                  o['rgb_marched'], o['rgb_pre'], o['cum_weights'], o['depth_acc'], None)
    ops.loss_rays(o['rgb_marched'], o['alphainv_last'], o['cum_weights'], d['target'], d['mask'], o['mask_sum'], W_MAIN, W_ENT, W_MASK,
                  LS, o['g_rgbm'], o['g_last'], o['g_cw'], o['loss'], None)
    ops.march_bwd(d['alpha'], d['rgb'], d['step'], o['weights'], o['T'], o['alphainv_last'], d['rs'], o['i_end'], d['N'], bg,
                  o['rgb_pre'], o['g_rgbm'], o['g_cw'], o['g_last'], None, None, o['g_alpha'], o['g_rgb'])
    torch.cuda.synchronize()
    return o


def run_fused(d, bg, work, cap=CAP, o=None):
    from poseprobe_amd import ops
    o = buffers(d) if o is None else o
    ops.march_loss_bwd(d['alpha'], d['rgb'], d['step'], d['rs'], d['N'], cap, bg, o['weights'], o['T'], o['alphainv_last'], o['i_end'],
                       o['rgb_marched'], o['rgb_pre'], o['cum_weights'], o['depth_acc'], d['target'], d['mask'], o['mask_sum'], W_MAIN,
                       W_ENT, W_MASK, LS, o['g_rgbm'], o['g_last'], o['g_cw'], o['loss'], None, None, o['g_alpha'], o['g_rgb'], work)
    torch.cuda.synchronize()
    return o


def loss_float64(d, o):
    """The four ray-loss values from the per-ray terms of k_loss_rays - evaluated in float32 in the kernel's order of operations on
    the composited values `o` holds - added up and normalised in float64."""
    rgbm, a, c0 = (o[k].cpu().numpy() for k in ('rgb_marched', 'alphainv_last', 'cum_weights'))
    tgt, y = d['target'].cpu().numpy(), d['mask'].cpu().numpy()
    diff = rgbm * y[:, None] - tgt * y[:, None]
    sq = diff * diff
    l_mse = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
    one = F32(1.0)
    p = np.minimum(np.maximum(a, F32(1e-6)), one - F32(1e-6))
    l_ent = -(p * np.log(p) + (one - p) * np.log(one - p))
    c = np.minimum(np.maximum(c0, F32(1e-3)), one - F32(1e-3))
    l_bce = -(y * np.log(c) + (one - y) * np.log(one - c))
    assert l_mse.dtype == l_ent.dtype == l_bce.dtype == np.float32
    n, msum = float(d['N']), float(y.astype(np.float64).sum())
    mse, ent, bce = l_mse.astype(np.float64).sum() / (msum * 3.0), l_ent.astype(np.float64).sum() / n, l_bce.astype(np.float64).sum() / n
    return np.array([mse, ent, bce, W_MAIN * mse + W_ENT * ent + W_MASK * bce])


def loss_distance(d, o, ref64):
    """Largest relative distance of the four values of o['loss'] from the float64 sums."""
    got = o['loss'].cpu().numpy().astype(np.float64)[list(SLOTS)]
    return float(np.max(np.abs(got - ref64) / np.abs(ref64)))


# Distance of pp_loss_rays from the float64 sum of the same per-ray terms on these inputs (largest relative distance over the four
# values, larger of two runs; MI355X), measured before the tolerance was fixed.  The fused kernel adds the same terms in another
# tree, so it is allowed twice that distance.
LOSS_DISTANCE = {('seven', 0.0): 1.464e-7, ('seven', 0.5): 1.464e-7, ('many', 0.0): 6.825e-8, ('many', 0.5): 7.387e-8}


def same_bits(a, b, what):
    a, b = a.cpu(), b.cpu()
    ai, bi = (a.view(torch.int32), b.view(torch.int32)) if a.is_floating_point() else (a, b)
    assert bool((ai == bi).all()), f'{what}: {int((ai != bi).sum())} of {a.numel()} entries differ from the separate launches'


def workspace(d, cap=CAP):
    from poseprobe_amd import ops
    return torch.zeros(ops.march_loss_workspace(d['N'], cap), dtype=torch.uint8, device='cuda')


@pytest.mark.parametrize('bg', [0.0, 0.5])
@pytest.mark.parametrize('name', ['seven', 'many'])
def test_fused_ray_launch_equals_the_separate_launches(name, bg):
    """seven: 7 rays (two work-groups, the second ragged) of 0, 1, 63, 64, 65, 129 and 186 samples.  many: 261 rays of 0 .. 186 samples,
    66 work-groups, so the last one to arrive has rows to add in more than one wavefront.  Both hold rays that stop early inside the
    first chunk, exactly at a chunk boundary (i_end = ray start + 64), in the last chunk and never; colours that composite outside
    [0, 1]; mask pixels 0 and 1; alphainv_last and cum_weights inside and outside their clamp ranges (checked below).
    Loss values: LOSS_DISTANCE holds the measured relative distance of pp_loss_rays from the float64 sums for each case; the fused
    kernel is allowed twice that.  Measured on an MI355X, largest relative distance over the four values (pp_loss_rays, the same in
    two runs / fused kernel, the same in two calls): seven, bg 0: 1.464e-7 / 1.464e-7; seven, bg 0.5: 1.464e-7 / 1.464e-7 (in both
    the entropy value, one float32 ulp; the fused kernel's bce value is 8.7e-8 off where pp_loss_rays' is 1.4e-8 off); many, bg 0:
    6.825e-8 / 8.339e-8; many, bg 0.5: 7.387e-8 / 8.339e-8."""
    d = make_case(name)
    sep = run_separate(d, bg)
    # the case holds what it says
    i_end, rs = sep['i_end'].cpu(), d['rs'].cpu()
    length = rs[1:] - rs[:-1]
    stop = i_end - rs[:-1]
    assert bool(((stop < length) & (stop < 64) & (length > 0)).any()), 'no early stop inside the first chunk'
    assert bool(((stop == 64) & (length > 64)).any()), 'no early stop at a chunk boundary'
    assert bool(((stop < length) & (stop > 128)).any()), 'no early stop in the last chunk'
    assert bool(((stop == length) & (length > 128)).any()), 'no three-chunk ray without an early stop'
    pre, al, cw = sep['rgb_pre'].cpu(), sep['alphainv_last'].cpu(), sep['cum_weights'].cpu()
    assert bool((pre < 0).any()) and bool((pre > 1).any()) and bool(((pre >= 0) & (pre <= 1)).any())
    assert bool((al < 1e-6).any()) and bool((al > 1 - 1e-6).any()) and bool(((al > 1e-6) & (al < 1 - 1e-6)).any())
    assert bool((cw < 1e-3).any()) and bool((cw > 1 - 1e-3).any()) and bool(((cw > 1e-3) & (cw < 1 - 1e-3)).any())
    assert bool((sep['g_rgbm'].cpu() != 0).any()) and bool((sep['g_alpha'][:d['M']].cpu() != 0).any())

    work = workspace(d)
    fus = run_fused(d, bg, work)
    for k in PER_SAMPLE + PER_RAY:
        same_bits(fus[k], sep[k], k)                     # whole buffers: the 64 entries behind the last sample keep their fill
    assert int(work.view(torch.int32)[0]) == 0, 'ticket not left zero'

    ref64 = loss_float64(d, sep)
    sep2 = run_separate(d, bg)
    d_parent = max(loss_distance(d, sep, ref64), loss_distance(d, sep2, ref64))
    d_fused = loss_distance(d, fus, ref64)
    print(f'{name} bg={bg}: pp_loss_rays {d_parent:.3e}, fused {d_fused:.3e}, allowed {2 * LOSS_DISTANCE[(name, bg)]:.3e} '
          f'(relative distance from the float64 sums)')
    others = [i for i in range(8) if i not in SLOTS]
    assert float(fus['loss'][others].abs().max()) == 0.0
    # the recorded figure is still what pp_loss_rays gives on these inputs (it would move with the inputs or with that kernel)
    assert abs(d_parent - LOSS_DISTANCE[(name, bg)]) <= 1e-3 * LOSS_DISTANCE[(name, bg)]
    assert d_fused <= 2 * LOSS_DISTANCE[(name, bg)]

    # a second call on the same workspace: the same bits, loss values included (fixed order), ticket zero again
    again = run_fused(d, bg, work)
    for k in PER_SAMPLE + PER_RAY + ('loss',):
        same_bits(again[k], fus[k], f'second call: {k}')
    assert int(work.view(torch.int32)[0]) == 0


def test_a_longer_ray_than_the_kernel_holds_is_refused():
    """The kernel keeps three chunks of a ray in registers: sample_cap = 193 is refused by the workspace query and by the launch, which
    writes nothing."""
    from poseprobe_amd import ops
    from poseprobe_amd._lib import PoseProbeError
    d = make_case('seven')
    with pytest.raises(PoseProbeError, match='192'):
        ops.march_loss_workspace(d['N'], 193)
    work = workspace(d)
    work.fill_(9)
    o = buffers(d)
    o['loss'].fill_(-77.0)
    with pytest.raises(PoseProbeError, match='192'):
        run_fused(d, 0.0, work, cap=193, o=o)
    torch.cuda.synchronize()
    for k, t in o.items():
        assert bool((t == (-7 if k == 'i_end' else -77.0)).all()), f'{k} was written'
    assert bool((work == 9).all())
    ops.march_loss_workspace(d['N'], 192)

